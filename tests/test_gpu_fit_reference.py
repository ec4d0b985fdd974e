"""The four fit kernels -- the register kernel pf_fit_reg_kernel<KPAD, RPT, 256>, the general kernel pf_fit_kernel<KPAD>, the TSQR
kernel pf_fit_tsqr_kernel<MC, RC> and the panel kernel pf_fit_panel_kernel<NT16, RPT, PW> -- against the extended-precision reference
of tests/fit_reference.py, at every plan the API can reach.  Every case asserts the single plan it ran by the delta of the host-side
launch counters (pfmi_kernel_time "fit:reg:..", "fit:gen:..", "fit:tsqr:..", "fit:panel:..", include/pfmi.h) and checks EVERY fit of
the case, not a sample of trace points.  The cases are fit_reference.GRID; tests/test_fit_reference_cpu.py proves on the CPU that they
take every reachable plan and that the double oracle stays inside the same bounds with its own, longer chain.

What is asserted per fit (eps = 2^-52; the constants and their derivations are in the docstring of tests/fit_reference.py):
  B, D against the long-double B and D of the kernel's own inputs; D's scale is the forward bound of the triangular inverse
  |Q_k (V'V - I) Q_k' - B~ D B~'|_ij <= C_W eps sqrt(S_ii S_jj), from the fit's own (sqrt_alpha, reflectors, T, V) and its own B, D:
      the factor's backward error.  No conditioning gate, no cond(D) allowance: it holds at a rank-deficient block
  |Q_k'Q_k - I| <= C_Q eps, logdet and mu against the reference; status, j_eff and n_rejected array-equal with the oracle's walk
d <= 256: every entry of the d x d backward error; above: every column of the rows fit_reference.check_rows names."""
import json

import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import fit_reference as fr                                     # noqa: E402
import margins as mg                                           # noqa: E402

pytestmark = pytest.mark.gpu

_SEEN = set()
_DONE = set()
HOOK = "PFMI_FIT_KERNEL"


def _counts(eng):
    return {nm: eng.kernel_time(nm)[1] for nm in fr.ALL_PLANS}


def _fit_asserting(eng, monkeypatch, J, expect, force):
    """fit_batch(J) (under PFMI_FIT_KERNEL=force) and the assertion that exactly one fit kernel was launched, of plan `expect`"""
    before = _counts(eng)
    if force:
        monkeypatch.setenv(HOOK, force)
    else:
        monkeypatch.delenv(HOOK, raising=False)
    try:
        eng.fit_batch(J)
    finally:
        monkeypatch.delenv(HOOK, raising=False)
    after = _counts(eng)
    delta = {k: after[k] - before[k] for k in fr.ALL_PLANS if after[k] != before[k]}
    assert delta == {expect: 1}, (delta, expect)
    assert eng.kernel_time("fit:")[1] == 0                     # an unknown plan name counts nothing
    _SEEN.add(expect)


def _load(pfmi, eng, c):
    th, gr, walks = fr.oracle_walk(c)
    eng.set_target(pfmi.t_iso(c.d))
    eng.set_traces(th, gr)
    return th, gr, walks


def _run_case(pfmi, eng, monkeypatch, i):
    if i in _DONE:
        return
    c = fr.GRID[i]
    plan = fr.case_plan(c)
    th, gr, walks = _load(pfmi, eng, c)
    _fit_asserting(eng, monkeypatch, c.J, plan, c.force)
    status, jeff, logdet, nrej = eng.fit_status()
    assert eng.P == sum(c.lengths)
    np.testing.assert_array_equal(jeff, np.concatenate([w[1] for w in walks]))
    np.testing.assert_array_equal(nrej, [w[3] for w in walks])
    np.testing.assert_array_equal(status, np.zeros(eng.P, dtype=np.int32))          # the oracle's: every pair accepted is s'y > 0
    rows = fr.check_rows(c.d, plan)
    worst, raw, failures, dep = {}, {}, [], 0
    for k, (t, g, (al, hl, hs, rej)) in enumerate(zip(th, gr, walks)):
        for l in range(len(t)):
            p = int(eng.offsets[k]) + l
            j = int(hl[l])
            f = eng.get_fit(p, j)
            assert f["logdet"] == logdet[p] or (np.isnan(f["logdet"]) and np.isnan(logdet[p]))
            S, Y = fr.history_columns(t, g, hs[l, :j])
            ref = fr.FitRef(f["alpha"], S, Y, t[l], g[l])      # alpha as the device's history walk left it
            assert ref.sign == 1
            rep, bad = fr.fit_report(f, ref, plan, rows)
            for nm, (v, C) in rep.items():
                mg.record(plan, f"fit_{nm}_eps@gpu_vs_ld", v, C)
                if v / C >= worst.get(nm, -1.0):
                    worst[nm], raw[nm] = v / C, v
            if bad:
                failures.append((k, l, j, bad))
            dep += j > 0 and fr.qr_ratio(f) < 1e-4
    print(json.dumps({"case": fr.case_id(c), "plan": plan, "fits": int(eng.P), "dependent_fits": int(dep),
                      "largest_ratio_over_C": {nm: float(f"{v:.3g}") for nm, v in worst.items()},
                      "largest_ratio": {nm: float(f"{v:.3g}") for nm, v in raw.items()}}))
    assert not failures, (fr.case_id(c), plan, failures)
    _DONE.add(i)


# ---- 1. every plan, every fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(fr.GRID)), ids=[fr.case_id(c) for c in fr.GRID])
def test_fit_every_plan_matches_the_reference(pfmi_mod, eng, monkeypatch, i):
    """the register kernel at every (KPAD, RPT) and RPT edge, the general kernel where it is the default and forced, the TSQR and the panel
    kernel at every KPAD, chunk and bucket boundary, scaled rows, nearly dependent steps, 2 j > d, a non-finite gradient component: the
    plan counter named by fit_reference.plan_for rises by one, no other fit counter moves, and every fit of the case passes check_fit"""
    _run_case(pfmi_mod, eng, monkeypatch, i)


# ---- 2. stale padding --------------------------------------------------------------------------------------------------------------------
REFIT = [(257, 3, "dep", None), (65, 9, "scaled", None), (1025, 4, "dep", None)]          # fit:reg:8,2  fit:gen:20  fit:tsqr:8


def _snapshot(eng, jeff, X):
    out = [np.asarray(v).tobytes() for v in eng.fit_status()]
    for p in range(eng.P):
        f = eng.get_fit(p, int(jeff[p]))
        out += [np.asarray(f[nm]).tobytes() for nm in ("alpha", "B", "D", "qr_factors", "T", "V", "mu")] + [np.float64(f["logdet"]).tobytes()]
        out.append(eng.logpdf(p, X).tobytes())
        # the operator surface reads the same padding: mode 3 back-substitutes through the identity padding of V, mode 1 divides by its
        # padded diagonal, every mode contracts over the padded columns of Vh and T, diag over the padding of D
        out += [np.asarray(eng.woodbury_apply(p, op, X)).tobytes() for op in _ops(eng)]
        out.append(eng.woodbury_diag(p).tobytes())
    return out


def _ops(eng):
    ops = sorted(eng.OPS, key=eng.OPS.get)
    assert len(ops) == 8
    return ops


@pytest.mark.parametrize("d,J,regime,force", REFIT, ids=[fr.plan_for(d, J, f) for d, J, _, f in REFIT])
def test_refit_on_a_used_context_is_bit_identical(pfmi_mod, eng, monkeypatch, d, J, regime, force):
    """the padding of Vh, T, V and D (columns 2 j .. KPAD, rows beyond k) is read by the scan, the density kernels and the operator surface
    (pfmi_woodbury_apply, pfmi_woodbury_diag) but is invisible through pfmi_get_fit.  On an engine that has just fitted a full J = 8
    history of the same d (KPAD = 16: another layout, every slot written) the case's fits, statuses, densities, all eight operators at 8
    columns and diag must be the bits a fresh engine gives."""
    c = fr.make_case(d, J, regime, 900 + d)
    plan = fr.plan_for(d, J, force)
    X = np.random.default_rng(d).normal(size=(d, 8))
    prev = fr.make_case(d, 8, "plain", 901 + d, points=sum(c.lengths) // 2 + 8)
    _load(pfmi_mod, eng, prev)
    _fit_asserting(eng, monkeypatch, 8, fr.plan_for(d, 8), None)
    _load(pfmi_mod, eng, c)
    _fit_asserting(eng, monkeypatch, J, plan, force)
    jeff = eng.fit_status()[1]
    used = _snapshot(eng, jeff, X)
    fresh = pfmi_mod.Engine(0)
    try:
        _load(pfmi_mod, fresh, c)
        _fit_asserting(fresh, monkeypatch, J, plan, force)
        new = _snapshot(fresh, jeff, X)
    finally:
        fresh.close()
    assert len(used) == len(new)
    differ = [i for i, (a, b) in enumerate(zip(used, new)) if a != b]
    assert not differ, (plan, differ[:8])


# ---- 3. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_union_of_plans_run_equals_reachable(pfmi_mod, eng, monkeypatch):
    """every reachable plan of the CPU mirror was launched by this module (the grid cases run here if they have not run yet), and nothing
    outside the mirror's list was"""
    for i in range(len(fr.GRID)):
        _run_case(pfmi_mod, eng, monkeypatch, i)
    assert _SEEN == set(fr.REACHABLE), (sorted(set(fr.REACHABLE) - _SEEN), sorted(_SEEN - set(fr.REACHABLE)))
    counts = _counts(eng)
    assert not [nm for nm in fr.EXCLUDED if counts.get(nm)]
