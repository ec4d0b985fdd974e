"""Pins tests/fit_reference.py on the CPU: the double oracle (oracle/pf_oracle.c) goes through check_fit on the whole grid of
tests/test_gpu_fit_reference.py and must stay inside every bound (with L = d, its row-after-row chain); eight wrong fits must each
exceed the bound they target; the Python mirror of the fit dispatch must send the grid to exactly the reachable plans; and the factor
bound, which has no conditioning gate, must see nearly rank-deficient blocks in every kernel family.  CPU only."""
import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import fit_reference as fr                                     # noqa: E402

_RES = {}


def _run_case(i):
    """every fit of grid case i through the oracle and the reference: {"ratios": {name: largest ratio / C}, "dep": number of fits with
    QR diagonal ratio < 1e-4 that passed the factor bound, "fits": number of fits checked}"""
    if i in _RES:
        return _RES[i]
    c = fr.GRID[i]
    th, gr, walks = fr.oracle_walk(c)
    plan = fr.case_plan(c)
    rows = fr.check_rows(c.d, plan)
    worst, dep, n = {}, 0, 0
    for k, (t, g, (al, hl, hs, rej)) in enumerate(zip(th, gr, walks)):
        if c.bad is None:
            assert rej == 0 and list(hl) == [min(l, c.J) for l in range(len(t))], (fr.case_id(c), rej, list(hl))
        for l in range(len(t)):
            j = int(hl[l])
            S, Y = fr.history_columns(t, g, hs[l, :j])
            f, status = fr.oracle_fit(al[l], S, Y, t[l], g[l])
            assert status == 0, (fr.case_id(c), k, l, status)
            ref = fr.FitRef(al[l], S, Y, t[l], g[l])
            assert ref.sign == 1
            rel = fr.check_fit(f, ref, "oracle", rows, ctx=(fr.case_id(c), k, l))
            for nm, v in rel.items():
                worst[nm] = max(worst.get(nm, 0.0), v)
            dep += fr.qr_ratio(f) < 1e-4 and j > 0
            n += 1
    _RES[i] = {"ratios": worst, "dep": int(dep), "fits": n}
    return _RES[i]


@pytest.mark.parametrize("i", range(len(fr.GRID)), ids=[fr.case_id(c) for c in fr.GRID])
def test_oracle_stays_inside_every_bound(i):
    """the bounds are honest: a correct double implementation, summing row after row (L = d), passes B, D, W, Q, logdet and mu on every fit
    of every grid case -- the ramp j = 0 .. J, the wrapped ring, 2 j > d, scaled rows and nearly dependent steps"""
    r = _run_case(i)
    assert r["fits"] == sum(fr.GRID[i].lengths)


def test_nonfinite_gradient_rejects_the_two_pairs_that_touch_it():
    """NaN / Inf in one gradient component of point 3: n_rejected = 2 and j_eff stalls for two points, whatever the summation order"""
    for c in fr.GRID:
        if c.bad is None:
            continue
        _, _, walks = fr.oracle_walk(c)
        al, hl, hs, rej = walks[0]
        n = c.lengths[0]
        want = [min(l if l < 3 else 2 if l < 5 else l - 2, c.J) for l in range(n)]
        assert rej == 2 and list(hl) == want, (fr.case_id(c), rej, list(hl), want)
        for l in range(n):
            assert not ({2, 3} & set(int(v) for v in hs[l, :hl[l]])), (l, hs[l])      # pairs (2, 3) and (3, 4) never enter a history
        assert walks[1][3] == 0


def test_plan_for_over_the_grid_equals_reachable():
    seen = {fr.case_plan(c) for c in fr.GRID}
    assert seen == set(fr.REACHABLE), (sorted(seen - set(fr.REACHABLE)), sorted(set(fr.REACHABLE) - seen))
    assert set(fr.REACHABLE) | set(fr.EXCLUDED) == set(fr.ALL_PLANS) and len(set(fr.ALL_PLANS)) == len(fr.ALL_PLANS) == 44


def test_dispatch_mirror_at_the_route_boundaries():
    """the thresholds of pf_launch_fit, launch_fit_t, pf_launch_fit_tsqr and pf_launch_fit_panel, and what PFMI_FIT_KERNEL changes"""
    P = fr.plan_for
    assert [P(d, 4) for d in (256, 257, 512, 513, 1024, 1025)] == ["fit:reg:8,1", "fit:reg:8,2", "fit:reg:8,2", "fit:reg:8,4", "fit:reg:8,4",
                                                                  "fit:tsqr:8"]
    assert P(1024, 9) == "fit:gen:20" and P(1025, 10) == "fit:tsqr:20" and P(1024, 4, "mem") == "fit:gen:8"
    assert P(1024, 4, "tsqr") == P(1024, 4, "panel") == "fit:reg:8,4"                     # the large-d hooks do nothing at d <= 1024
    assert P(1025, 2) == P(1025, 2, "panel") == "fit:gen:4" and P(2000, 17) == "fit:gen:64"
    assert P(4095, 16) == "fit:panel:32,10,4" and P(4096, 16) == "fit:tsqr:32" and P(1025, 16, "tsqr") == "fit:tsqr:32"
    assert P(16384, 16) == "fit:tsqr:32" and P(16385, 16) == "fit:gen:32"                  # 17 chunks x 32 rows > the stack; past the panel kernel
    assert P(32768, 4) == "fit:tsqr:8" and P(32769, 4) == "fit:gen:8"
    assert [P(d, 4, "panel") for d in (2560, 2561, 5120, 5121, 10240, 10241, 16384, 16385)] == [
        "fit:panel:8,5,4", "fit:panel:8,10,4", "fit:panel:8,10,4", "fit:panel:8,20,4", "fit:panel:8,20,4", "fit:panel:8,32,2",
        "fit:panel:8,32,2", "fit:gen:8"]
    assert P(3000, 6, "mem") == "fit:gen:12"


def _mutation_fit(d=513, J=4):
    th, gr = fr.quad_history(d, (J + 3,), 1e4, None, 7)
    al, hl, hs, _ = fr.po.lbfgs_history(th[0], gr[0], J)
    l = J + 2                                                  # a wrapped ring
    S, Y = fr.history_columns(th[0], gr[0], hs[l, :hl[l]])
    f, status = fr.oracle_fit(al[l], S, Y, th[0][l], gr[0][l])
    assert status == 0 and hl[l] == J
    return f, fr.FitRef(al[l], S, Y, th[0][l], gr[0][l])


MUTATION_FACTORS = {}


@pytest.mark.parametrize("name", list(fr.MUTATIONS))
def test_every_mutation_exceeds_the_bound_it_targets(name):
    """a d = 513, J = 4 fit (fit:reg:8,4 on the device) with one slip of the kind an RPT > 1 kernel could make: the unmutated fit passes
    check_fit, the mutated one exceeds the targeted bound -- also the loosest bound any implementation gets at this shape (L = d)"""
    f, ref = _mutation_fit()
    plan = fr.plan_for(513, 4)
    rows = fr.check_rows(513, plan)
    fr.check_fit(f, ref, "oracle", rows)
    g = fr.mutate(f, ref, name)
    which = fr.MUTATIONS[name]
    r = fr.fit_ratios(g, ref, rows)[which][0]
    loose, tight = fr.constants("oracle", 513, 4)[which], fr.constants(plan, 513, 4)[which]
    MUTATION_FACTORS[name] = (which, r / loose, r / tight)
    print(f"mutation {name}: {which} ratio {r:.3g} = {r / loose:.3g} x the oracle's bound, {r / tight:.3g} x the kernel's")
    assert r > loose >= tight, (name, which, r, loose, tight)
    with pytest.raises(AssertionError):
        fr.check_fit(g, ref, plan, rows)


def test_the_factor_bound_sees_dependent_blocks_in_every_family():
    """no conditioning gate: the fits with QR diagonal ratio below 1e-4 (the ones tests/gpu_common.py::_well_conditioned turns away) that
    pass the factor bound, per kernel family"""
    dep = {"reg": 0, "gen": 0, "tsqr": 0, "panel": 0}
    per_inst = {}
    for i, c in enumerate(fr.GRID):
        n = _run_case(i)["dep"]
        dep[fr.family(fr.case_plan(c))] += n
        if fr.family(fr.case_plan(c)) == "reg":
            per_inst[fr.case_plan(c)] = per_inst.get(fr.case_plan(c), 0) + n
    assert all(v >= 1 for v in dep.values()), dep
    assert len(per_inst) == 12 and all(v >= 1 for v in per_inst.values()), per_inst      # every (KPAD, RPT) of the register kernel
