"""Pins tests/history_reference.py on the CPU: on every case of the grid of tests/test_gpu_history_steps.py the double oracle's walk
(oracle/pf_oracle.c, which divides and sums row after row) and a NumPy float64 mirror of the walk in the summation order and the
reciprocal form of the case's own plan go through check_path and must stay inside the counted bound; seven faults applied to a
correct walk must each be rejected; every step's decision margin must be 1000 times the counted error of the comparison and no x_i may
cancel below half the sum of its terms; and the Python mirror of the dispatch must send the grid to exactly the 17 plans.  CPU only."""
import json

import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import history_reference as hr                                 # noqa: E402
import margins as mg                                           # noqa: E402
from oracle import pf_oracle as po                             # noqa: E402

_RES = {}
WHY = "error / counted bound (tests/history_reference.py), largest over every coordinate of every accepted step, one entry per case"
IDS = [hr.case_id(c) for c in hr.GRID]


def _oracle_walks(c, th, gr, eps):
    po.set_hinit(c.hinit)
    try:
        return [po.lbfgs_history(t, g, hr.J, eps) for t, g in zip(th, gr)]
    finally:
        po.set_hinit("gilbert")


def _run_case(i):
    """grid case i through the oracle and the plan's mirror: the largest error / bound of each, the smallest decision margin in units of
    the counted bound, the smallest x_i quotient and the step counts"""
    if i in _RES:
        return _RES[i]
    c = hr.GRID[i]
    plan = hr.case_plan(c)
    th, gr = hr.case_traces(c)
    eps, reps = hr.case_replays(c, th, gr)
    out = {"oracle": 0.0, "mirror": 0.0, "x_cond": np.inf, "margin": np.inf, "accepted": 0, "rejected": 0, "plan": plan, "eps": eps}
    walks = _oracle_walks(c, th, gr, eps)
    for k, (t, g, rep) in enumerate(zip(th, gr, reps)):
        for who, pl, (al, hl, hs, rej) in (("oracle", "oracle", walks[k]), ("mirror", plan, hr.mirror_walk(t, g, hr.J, eps, c.hinit, plan))):
            r, fails = hr.check_path(rep, pl, al, hl, rej, hr.sblock_of(t, g, hl, hs))
            assert not fails, (hr.case_id(c), who, k, fails[:3])
            out[who] = max(out[who], r["ratio"])
            out["x_cond"] = min(out["x_cond"], r["x_cond"])
        out["accepted"] += r["accepted"]
        out["rejected"] += r["rejected"]
        fin = rep.finite
        if np.any(fin):
            out["margin"] = min(out["margin"], float(np.min(rep.margin[fin])) / max(hr.decision_bound(plan, c.d), hr.decision_bound("oracle", c.d)))
    _RES[i] = out
    return out


@pytest.mark.parametrize("i", range(len(hr.GRID)), ids=IDS)
def test_oracle_and_mirror_stay_inside_the_counted_bound(i):
    """the bound is honest: two correct double walks -- the oracle's (divisions, one serial chain of d) and the mirror of the case's plan
    (carried reciprocal or divisions, the kernel's thread map, butterfly and wave order) -- pass every coordinate of every step; and the
    inputs are fit to be checked without exemptions: decision margin >= 1000 x the counted error of b - eps q under BOTH summation
    orders, min |x_i| / (|T1| + |T2| + |T3|) >= 0.5 (d = 1: exactly 1 / 3 by identity, see history_reference)"""
    c = hr.GRID[i]
    r = _run_case(i)
    print(json.dumps({"case": IDS[i], "plan": r["plan"], "oracle_err_over_bound": float(f"{r['oracle']:.3g}"),
                      "mirror_err_over_bound": float(f"{r['mirror']:.3g}"), "margin_over_bound": float(f"{r['margin']:.3g}"),
                      "x_cond": float(f"{r['x_cond']:.3g}"), "accepted": r["accepted"], "rejected": r["rejected"]}))
    mg.record(r["plan"], "hist_alpha_bound@oracle_vs_ld", r["oracle"], 1.0, why=WHY + "; the double oracle on the plan's cases (chain d, divisions)")
    mg.record(r["plan"], "hist_alpha_bound@mirror_vs_ld", r["mirror"], 1.0, why=WHY + "; the float64 mirror in the plan's summation order")
    assert r["oracle"] < 1 and r["mirror"] < 1
    assert r["margin"] >= hr.MARGIN_FACTOR, (IDS[i], r["margin"])
    if c.hinit == "gilbert" and r["accepted"]:
        if c.d == 1:
            assert abs(r["x_cond"] - 1 / 3) < 1e-12, r["x_cond"]
        else:
            assert r["x_cond"] >= hr.X_COND_MIN, (IDS[i], r["x_cond"])
    steps = sum(n - 1 for n in hr.LENGTHS)
    assert r["accepted"] + r["rejected"] == steps
    if c.eps == "third":
        nbad = 2 if c.bad else 0
        assert r["rejected"] == (steps - nbad) // 3 + nbad, (r["rejected"], steps)     # the ring has gaps
    elif c.eps == "none":
        assert r["accepted"] == 0
    else:
        assert r["rejected"] == (2 if c.bad else 0)


def test_largest_ratio_per_plan_is_below_one():
    """the table of profiles/history_walk_parity.md: the largest error / bound of the oracle and of the mirror per plan"""
    per = {}
    for i in range(len(hr.GRID)):
        r = _run_case(i)
        o, m = per.get(r["plan"], (0.0, 0.0))
        per[r["plan"]] = (max(o, r["oracle"]), max(m, r["mirror"]))
    for plan in hr.ALL_PLANS:
        print(json.dumps({"plan": plan, "oracle": float(f"{per[plan][0]:.3g}"), "mirror": float(f"{per[plan][1]:.3g}")}))
    assert set(per) == set(hr.ALL_PLANS)
    assert max(max(v) for v in per.values()) < 1


MUT_CASES = [hr.Case(513, None, "scaled", 41), hr.Case(5000, None, "plain", 42), hr.Case(130, None, "dep", 43)]
WANT = {"drop_last_coordinate": {"alpha"}, "alpha_two_points_back": {"alpha"}, "stale_reciprocal": {"alpha"}, "c_replaced_by_a": {"alpha"},
        "rejected_step_applied": {"rejected_step_moved_alpha", "j_eff", "n_rejected"}, "last_step_not_applied": {"alpha", "j_eff", "n_rejected"},
        "ring_source_off_by_one": {"ring_sources"}}


def _mut_path(reps):
    """the path of a case with the most evenly mixed decisions"""
    return int(np.argmax([min(r.n_rejected, r.n - 1 - r.n_rejected) for r in reps]))


@pytest.mark.parametrize("mut", hr.MUTATIONS)
def test_every_mutation_is_rejected(mut):
    """one fault in an otherwise correct walk of the plan's own summation order: the checker fails the path, by the assertion the fault
    is aimed at, on a <4, 256> register case, a lean case and a single-wave case; the unmutated walk of the same inputs passes"""
    assert set(WANT) == set(hr.MUTATIONS)
    for c in MUT_CASES:
        plan = hr.case_plan(c)
        th, gr = hr.case_traces(c)
        eps, reps = hr.case_replays(c, th, gr)
        k = _mut_path(reps)
        t, g, rep = th[k], gr[k], reps[k]
        assert rep.n_rejected >= 3 and rep.n - 1 - rep.n_rejected > hr.J      # steps are rejected mid-trace and the ring wraps
        al, hl, hs, rej = hr.mirror_walk(t, g, hr.J, eps, c.hinit, plan)
        assert not hr.check_path(rep, plan, al, hl, rej, hr.sblock_of(t, g, hl, hs))[1]
        if mut == "last_step_not_applied" and not rep.accept[-1]:
            continue                                            # (a rejected last step: leaving it out changes nothing)
        al, hl, hs, rej = hr.mirror_walk(t, g, hr.J, eps, c.hinit, plan, mut)
        _, fails = hr.check_path(rep, plan, al, hl, rej, hr.sblock_of(t, g, hl, hs))
        kinds = {f[0] for f in fails}
        assert kinds & WANT[mut], (hr.case_id(c), mut, kinds)
        if mut == "ring_source_off_by_one":
            assert kinds == {"ring_sources"}                    # nothing else sees the ring's sources


@pytest.mark.parametrize("brk", hr.KERNEL_BREAKS)
def test_every_kernel_break_is_rejected_on_the_mirror(brk):
    """the three slips of pf_history_kernel that the fit-stage reference cannot see (it takes alpha as the walk left it), restated on the
    mirror of a register plan whose d leaves empty slots and whose L is no multiple of the unroll: each fails check_path through alpha"""
    hits = 0
    for c in MUT_CASES:
        plan = hr.case_plan(c)
        th, gr = hr.case_traces(c)
        eps, reps = hr.case_replays(c, th, gr)
        for k, (t, g, rep) in enumerate(zip(th, gr, reps)):
            ns = 4 if hr.geometry(plan, c.d)[1] <= 6 else 3
            tail = (rep.n - 1) % ns
            if rep.n < hr.J + 6 or not np.any(rep.accept[rep.n - 1 - tail if brk == "tail_dropped" else 0:]):
                continue                                        # (no accepted step, or none in the dropped tail: nothing to see)
            al, hl, hs, rej = hr.mirror_walk(t, g, hr.J, eps, c.hinit, plan, brk)
            _, fails = hr.check_path(rep, plan, al, hl, rej, hr.sblock_of(t, g, hl, hs))
            assert "alpha" in {f[0] for f in fails}, (hr.case_id(c), brk, k, fails[:3])
            hits += 1
    assert hits >= 3


def test_last_step_mutation_meets_an_accepted_last_step():
    """the remainder of the unrolled loop: at least one mutation case ends its longest path with an accepted step"""
    hit = 0
    for c in MUT_CASES:
        th, gr = hr.case_traces(c)
        _, reps = hr.case_replays(c, th, gr)
        hit += bool(reps[_mut_path(reps)].accept[-1])
    assert hit >= 1


def test_plan_for_over_the_grid_equals_reachable():
    seen = {hr.case_plan(c) for c in hr.GRID}
    assert seen == set(hr.REACHABLE), (sorted(seen - set(hr.REACHABLE)), sorted(set(hr.REACHABLE) - seen))
    assert len(hr.ALL_PLANS) == len(set(hr.ALL_PLANS)) == 17
    P = hr.plan_for
    assert [P(d) for d in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == [
        "hist:reg:1,64", "hist:reg:1,64", "hist:reg:2,64", "hist:reg:2,64", "hist:reg:4,64", "hist:reg:4,64", "hist:reg:2,256", "hist:reg:2,256",
        "hist:reg:4,256", "hist:reg:4,256", "hist:reg:2,1024", "hist:reg:2,1024"]
    assert [P(d) for d in (2049, 4096, 4097, 6144, 6145, 8192, 8193, 10240)] == [f"hist:lean:{e}" for e in (4, 4, 6, 6, 8, 8, 10, 10)]
    assert [P(d, "prefetch") for d in (2049, 4097, 6145, 10240)] == [f"hist:reg:{e},1024" for e in (4, 6, 8, 10)]
    assert [P(d) for d in (10241, 12288, 12289, 16384, 16385)] == ["hist:reg:12,1024"] * 2 + ["hist:reg:16,1024"] * 2 + ["hist:mem"]
    assert P(1, "mem") == P(2049, "mem") == "hist:mem" and P(1024, "prefetch") == "hist:reg:4,256" and P(2048, "prefetch") == "hist:reg:2,1024"
    assert P(12000, "prefetch") == "hist:reg:12,1024"
    # every instance at the lowest and the highest d of its range; the memory-resident kernel at its default and forced
    for lo, hi in hr.RANGES:
        assert {lo, hi} <= {c.d for c in hr.GRID if c.force is None and c.eps in ("third", "all")}
    assert {c.d for c in hr.GRID if c.force == "mem"} >= {1, 1023, 2049} and any(c.d == 16385 and c.force is None for c in hr.GRID)
    for fam, (d, force) in hr.FAMILY_CASES.items():
        got = [(c.eps, c.hinit, c.bad is not None) for c in hr.GRID if (c.d, c.force) == (d, force)]
        assert ("default", "gilbert", False) in got and ("third", "nocedal_wright", False) in got and ("third", "gilbert", True) in got, fam
