"""The Woodbury operator surface (pathfinder.jl_amd/csrc/woodbury_kernels.hip: pfmi_woodbury_apply's eight ops and pfmi_woodbury_diag)
against the long-double reference of tests/woodbury_reference.py, at all 28 instantiations of pf_woodbury_kernel<KPAD, MODE> and all 7
of pf_woodbury_diag_kernel<KPAD>.  The bounds are derived in woodbury_reference's docstring; tests/test_woodbury_reference_cpu.py pins
them on the CPU.  Fits come by the cheap route of tests/test_gpu_fit_reference.py (synthetic traces, no optimisation, no closure).

1. grid    J in {2, 4, 6, 8, 10, 16, 32} (every KPAD) x d in {2, KPAD - 1, KPAD, KPAD + 1, 300}; `plain` everywhere, `scaled` and `dep`
           at KPAD 12 and 32.  Every fit of a case at d <= KPAD + 1, the points {0, 1, J // 2, J, last} of each trace at d = 300; a case
           must hold a fit with j_eff = 0, one with 0 < j_eff < J, one with j_eff = J and, at d < 2 J, one with 2 j_eff > d.  All eight
           ops and diag on 9 columns (Gaussian entries, log-normal magnitudes); the two solves by their long-double residual through the
           forward operator, with no conditioning gate and no exemption list.  Every call asserts the launch counters' exact deltas.
2. lanes   N in {1, 255, 256, 257}: column n of an N-column call has the bits of the N = 1 call, and so has the vector form.
3. special an all-zero column gives exact zeros (+0.0 for the quadratic forms), NaN and inf stay in their own columns.
4. failed  every op and diag return NaN in every entry for a fit whose status is not PFMI_FIT_OK.
5. stale padding: tests/test_gpu_fit_reference.py::test_refit_on_a_used_context_is_bit_identical (its snapshot holds every op and diag).
6. coverage: all 28 + 7 counters counted, no unknown name counts.
Largest ratios seen: profiles/woodbury_parity.md."""
import json

import numpy as np
import pytest

from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

if not HAVE_LONGDOUBLE:
    pytest.skip(SKIP_REASON, allow_module_level=True)

import fit_reference as fr                                     # noqa: E402
import hmc_reference as H                                      # noqa: E402
import margins as mg                                           # noqa: E402
import woodbury_reference as W                                 # noqa: E402
from helpers import make_traces                                # noqa: E402

pytestmark = pytest.mark.gpu

_DONE = set()
_LAUNCHED = {}                                                 # plan name -> launches this module has asserted


def _load(pfmi, eng, c):
    th, gr, walks = fr.oracle_walk(c)
    eng.set_target(pfmi.t_iso(c.d))
    eng.set_traces(th, gr)
    return th, gr, walks


def _counts(eng, names):
    return {nm: eng.kernel_time(nm)[1] for nm in names}


def _counted(eng, kpad, expect, call):
    """call() with the assertion that the surface's counters of this KPAD moved by exactly `expect` ({name: launches})"""
    names = ["woodbury:%d:%d" % (kpad, m) for m in range(4)] + ["woodbury_diag:%d" % kpad]
    before = _counts(eng, names)
    out = call()
    after = _counts(eng, names)
    delta = {nm: after[nm] - before[nm] for nm in names if after[nm] != before[nm]}
    assert delta == expect, (delta, expect)
    for nm, n in delta.items():
        _LAUNCHED[nm] = _LAUNCHED.get(nm, 0) + n
    return out


def _apply(eng, kpad, p, op, X):
    expect = {}
    for m in W.LAUNCHES[op]:
        expect["woodbury:%d:%d" % (kpad, m)] = expect.get("woodbury:%d:%d" % (kpad, m), 0) + 1
    return _counted(eng, kpad, expect, lambda: eng.woodbury_apply(p, op, X))


def _diag(eng, kpad, p):
    return _counted(eng, kpad, {"woodbury_diag:%d" % kpad: 1}, lambda: eng.woodbury_diag(p))


def _fit_case(pfmi, eng, case):
    c = W.grid_case(case)
    th, gr, walks = _load(pfmi, eng, c)
    eng.fit_batch(c.J)
    return c, th, gr, walks


def _run_case(pfmi, eng, case):
    cid = W.case_id(case)
    if cid in _DONE:
        return
    d, J, _ = case
    kpad = H.kpad_for(J)
    every = _counts(eng, W.plan_names())
    c, th, gr, walks = _fit_case(pfmi, eng, case)
    status, jeff, _, _ = eng.fit_status()
    np.testing.assert_array_equal(jeff, np.concatenate([w[1] for w in walks]))
    np.testing.assert_array_equal(status, np.zeros(eng.P, dtype=np.int32))      # the oracle's: every fit of the case is checked below
    points = W.grid_points(case, c.lengths)
    got_j = [int(jeff[int(eng.offsets[k]) + l]) for k, l in points]
    for what, pred in W.grid_needs(case).items():
        assert any(pred(j) for j in got_j), (cid, what, got_j)
    worst = {}
    for k, l in points:
        p = int(eng.offsets[k]) + l
        j = int(jeff[p])
        f = eng.get_fit(p, j)
        ops = W.Ops(H.Metric.from_fit(f, dtype=W.LD))
        X = W.grid_X(case, p)
        r = {}
        for op in W.OPS:
            r.update(W.op_ratios(ops, kpad, op, X, _apply(eng, kpad, p, op, X)))
        S, Y = fr.history_columns(th[k], gr[k], walks[k][2][l, :j])
        r.update(W.diag_ratio(kpad, _diag(eng, kpad, p), f["alpha"], S, Y, f["D"]))
        assert set(r) == set(W.CHECKS)
        for q, v in r.items():
            mg.record("woodbury:%d" % kpad, "wb_" + q, [v], 1.0)
            if v >= worst.get(q, (-1.0,))[0]:
                worst[q] = (v, k, l, j)
    print("WOODBURY_GPU", json.dumps({"case": cid, "kpad": kpad, "fits": len(points),
                                      "largest_ratio": {q: float("%.3g" % v[0]) for q, v in worst.items()}}))
    for q, v in worst.items():                                  # every fit is recorded above; asserted on the case's largest, after the print
        mg.check("woodbury:%d" % kpad, "wb_" + q, [v[0]], 1.0, ctx=(cid,) + v[1:])
    after = _counts(eng, W.plan_names())
    n = len(points)
    expect = {"woodbury:%d:%d" % (kpad, m): n * sum(W.LAUNCHES[op].count(m) for op in W.OPS) for m in range(4)}
    expect["woodbury_diag:%d" % kpad] = n
    assert {nm: after[nm] - every[nm] for nm in after if after[nm] != every[nm]} == expect, cid      # and no other instantiation ran
    _DONE.add(cid)


# ---- 1. the grid -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.GRID, ids=[W.case_id(c) for c in W.GRID])
def test_every_op_is_inside_its_bound_at_every_fit(pfmi_mod, eng, case):
    _run_case(pfmi_mod, eng, case)


def _one_fit(pfmi, eng, kpad):
    """the last fit (j_eff = J) of the d = KPAD + 1 grid case: head block, one tail row, a full V"""
    J = kpad // 2
    case = (kpad + 1, J, "plain")
    c, _, _, _ = _fit_case(pfmi, eng, case)
    status, jeff, _, _ = eng.fit_status()
    p = c.lengths[0] - 1
    assert status[p] == 0 and jeff[p] == J
    return case, p


# ---- 2. lane independence and the block edge ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpad", W.KPADS)
def test_a_column_does_not_depend_on_its_neighbours_or_its_block(pfmi_mod, eng, kpad):
    case, p = _one_fit(pfmi_mod, eng, kpad)
    d = case[0]
    rng = np.random.default_rng(kpad)
    X = np.asfortranarray(rng.standard_normal((d, 257)) * np.exp(rng.standard_normal((d, 257))))
    for op in W.OPS:
        single = np.stack([np.asarray(_apply(eng, kpad, p, op, X[:, n:n + 1])) for n in range(257)], axis=-1)
        single = single.reshape(-1, 257)                        # (d, 257), or (1, 257) for the quadratic forms
        for N in (1, 255, 256, 257):
            got = np.asarray(_apply(eng, kpad, p, op, X[:, :N])).reshape(-1, N)
            assert got.tobytes() == np.ascontiguousarray(single[:, :N]).reshape(-1, N).tobytes(), (op, N)
        vec = np.asarray(_apply(eng, kpad, p, op, X[:, 3].copy()))
        assert vec.shape == (() if op in ("quad", "invquad") else (d,))
        assert vec.tobytes() == np.ascontiguousarray(single[:, 3]).tobytes(), op


# ---- 3. special values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpad", W.KPADS)
def test_zero_nan_and_inf_columns(pfmi_mod, eng, kpad):
    case, p = _one_fit(pfmi_mod, eng, kpad)
    d = case[0]
    rng = np.random.default_rng(100 + kpad)
    X = np.asfortranarray(rng.standard_normal((d, 6)))
    X[:, 1] = 0.0
    X[d // 2, 3] = np.nan
    X[d - 1, 5] = np.inf
    plain = [0, 2, 4]
    for op in W.OPS:
        got = np.asarray(_apply(eng, kpad, p, op, X)).reshape(-1, 6)
        ref = np.asarray(_apply(eng, kpad, p, op, np.asfortranarray(X[:, plain]))).reshape(-1, 3)
        assert np.ascontiguousarray(got[:, plain]).tobytes() == np.ascontiguousarray(ref).tobytes(), op
        assert np.all(np.isfinite(ref)), op
        assert np.all(got[:, 1] == 0.0), (op, got[:, 1])
        if op in ("quad", "invquad"):
            assert not np.signbit(got[0, 1]), op
        assert not np.all(np.isfinite(got[:, 3])) and not np.all(np.isfinite(got[:, 5])), op


# ---- 4. a failed fit -------------------------------------------------------------------------------------------------------------------------------
def test_failed_fit_gives_nan_from_every_op_and_from_diag(pfmi_mod, eng):
    """the construction of tests/test_gpu_mixture.py: a random walk with negative-curvature pairs accepted by fit_batch(J, -1e300)"""
    d, J = 40, 5
    kpad = H.kpad_for(J)
    rng = np.random.default_rng(0)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(9, d)), 0), rng.normal(size=(9, d))
    tg = pfmi_mod.t_diag(d, seed=3)
    good = make_traces(tg, 1, 3)[0]
    eng.set_target(tg)
    eng.set_traces([bad_th, good.points], [bad_gr, good.gradients])
    eng.fit_batch(J, -1e300)
    status = eng.fit_status()[0]
    bad = [p for p in range(eng.P) if status[p] != 0]
    okp = [p for p in range(eng.P) if status[p] == 0]
    assert bad and okp, status                                  # neither half below can pass vacuously
    X = np.asfortranarray(np.random.default_rng(1).normal(size=(d, 5)))
    for p in bad:
        for op in W.OPS:
            assert np.all(np.isnan(_apply(eng, kpad, p, op, X))), (p, op)
        assert np.all(np.isnan(_diag(eng, kpad, p))), p
    for p in okp:
        for op in W.OPS:
            assert np.all(np.isfinite(_apply(eng, kpad, p, op, X))), (p, op)
        assert np.all(np.isfinite(_diag(eng, kpad, p))), p


# ---- 6. which instantiation ran ------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_was_launched_and_counted(pfmi_mod, eng):
    """the grid cases that have not run in this session (a selection, a split over workers) run here first: the assertions are always made"""
    for case in W.GRID:
        _run_case(pfmi_mod, eng, case)
    names = W.plan_names()
    assert len(names) == 35
    assert not [nm for nm in names if _LAUNCHED.get(nm, 0) <= 0]
    counts = _counts(eng, names)
    assert not [nm for nm in names if counts[nm] < _LAUNCHED[nm]]
    assert set(_LAUNCHED) == set(names)
    for unknown in ("woodbury:", "woodbury:24:0", "woodbury:12:4", "woodbury_diag:", "woodbury_diag:24"):
        assert eng.kernel_time(unknown)[1] == 0, unknown
