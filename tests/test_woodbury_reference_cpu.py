"""Pins tests/woodbury_reference.py on the CPU: the float64 mirror of the lane kernels inside every bound at every KPAD, at j in {0, a
partial j, J} and at d in {2, KPAD - 1, KPAD, KPAD + 1, 300} on synthetic factors of the fits' shapes (hmc_reference.random_metric), the
residual checks of the two solves at a V whose diagonal falls to 1e-7 with no conditioning gate, every injected fault rejected on a
small case, and the grid of tests/test_gpu_woodbury.py naming all 7 KPADs x 4 modes with the kinds of fit each case must contain.
CPU only."""
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


def _columns(d, n, rng):
    return rng.standard_normal((d, n)) * np.exp(2.0 * rng.standard_normal((d, n)))


def _history(M, j, rng):
    """a synthetic trace behind the factor's alpha for the diag kernel: j + 1 points, the pairs in order, a symmetric D"""
    theta, grad = rng.standard_normal((j + 1, M.d)), rng.standard_normal((j + 1, M.d))
    D = rng.standard_normal((2 * j, 2 * j))
    return theta, grad, np.arange(j), D + D.T


def _all_ratios(M, kpad, X, hist=None, fault=None):
    """{check: largest ratio} of the mirror's eight ops on the columns of X (and of its diag on `hist`) against the long-double bounds"""
    ops = W.Ops(M)
    out = {}
    for op in W.OPS:
        res = np.stack([W.mirror_op(M, kpad, op, X[:, n], fault) for n in range(X.shape[1])], axis=-1)
        out.update(W.op_ratios(ops, kpad, op, X, res))
    if hist is not None:
        theta, grad, src, D = hist
        S, Y = fr.history_columns(theta, grad, src)
        out.update(W.diag_ratio(kpad, W.mirror_diag(kpad, M.s ** 2, theta, grad, src, D, fault), M.s ** 2, S, Y, D))
    return out


@pytest.mark.parametrize("kpad", W.KPADS)
def test_mirror_is_inside_every_bound_at_every_padding_and_edge(kpad):
    J = kpad // 2
    worst = {}
    for j in (0, max(1, J // 2), J):
        for d in W.grid_dims(kpad):
            rng = np.random.default_rng(1000 * kpad + 10 * d + j)
            M = H.random_metric(d, j, rng)
            r = _all_ratios(M, kpad, _columns(d, 2, rng), _history(M, j, rng))
            assert set(r) == set(W.CHECKS)
            for q, v in r.items():
                mg.check("cpu:woodbury:%d" % kpad, "wb_" + q, [v], 1.0, ctx=(d, j))
                worst[q] = max(worst.get(q, 0.0), v)
    print("WOODBURY_MIRROR", json.dumps({"kpad": kpad, "largest_ratio": {q: float("%.3g" % v) for q, v in worst.items()}}))
    assert max(worst.values()) > 1e-4                           # the bounds are not vacuous


@pytest.mark.parametrize("d,j,kpad", [(5, 6, 12), (12, 6, 12), (40, 6, 12), (21, 10, 20), (64, 16, 32)])
def test_residual_checks_hold_at_an_ill_conditioned_V_without_a_gate(d, j, kpad):
    rng = np.random.default_rng(d + j)
    M = H.random_metric(d, j, rng)
    k = M.k
    M.V[np.arange(k), np.arange(k)] = np.logspace(0, -7, k)[rng.permutation(k)]
    r = _all_ratios(M, kpad, _columns(d, 3, rng))
    print("WOODBURY_ILL", json.dumps({"d": d, "j": j, "kpad": kpad, "ratios": {q: float("%.3g" % v) for q, v in r.items()}}))
    for q, v in r.items():
        mg.check("cpu:woodbury:ill:%d" % kpad, "wb_" + q, [v], 1.0, ctx=(d, j))


# fault -> (d, j, kpad) of a small case and the checks that must reject it
REJECTS = {"T_for_Tt": ((15, 6, 12), ("unwhiten", "rmul", "whiten", "invunwhiten", "mul", "solve", "quad", "invquad")),
           "V_for_Vt": ((15, 6, 12), ("unwhiten", "rmul", "mul", "quad")),
           "fwd_for_back": ((15, 6, 12), ("invunwhiten", "invunwhiten_fwd", "solve")),
           "no_sqrt_alpha": ((15, 6, 12), ("unwhiten", "rmul", "whiten", "invunwhiten", "mul", "solve", "quad", "invquad")),
           "sqrt_alpha_wrong_side": ((15, 6, 12), ("unwhiten", "rmul", "whiten", "invunwhiten", "mul", "solve", "quad", "invquad")),
           "head_guard_dropped": ((5, 6, 12), ("unwhiten", "rmul", "whiten", "invunwhiten", "mul", "solve", "quad", "invquad")),
           "tail_from_kpad_plus_1": ((15, 6, 12), ("unwhiten", "rmul", "whiten", "invunwhiten", "mul", "solve", "quad", "invquad")),
           "diag_offdiag_dropped": ((15, 6, 12), ("diag",))}


def test_every_fault_has_a_rejecting_case():
    assert set(REJECTS) == set(W.FAULTS)


@pytest.mark.parametrize("fault", W.FAULTS)
def test_bounds_reject_injected_fault(fault):
    (d, j, kpad), must = REJECTS[fault]
    rng = np.random.default_rng(3)
    M = H.random_metric(d, j, rng)
    X, hist = _columns(d, 2, rng), _history(M, j, rng)
    good = _all_ratios(M, kpad, X, hist)
    assert max(good.values()) <= 1.0, good
    bad = _all_ratios(M, kpad, X, hist, fault=fault)
    assert all(bad[q] > 1.0 for q in must), (fault, {q: bad[q] for q in must})


def test_constants_are_the_stated_counts():
    assert W.c_lane(300, 20) == 300 + 60 + 16 and W.c_solve(300, 20) == W.c_lane(300, 20) + 20 and W.c_diag(20) == 48
    assert W.EPS == 2.0 ** -52


def test_grid_names_every_instantiation_and_every_kind_of_fit():
    """all 7 KPADs x 4 modes and the 7 diag kernels; every d of grid_dims at every KPAD; and, by the oracle's history walk, each case
    holds and checks a fit with j_eff = 0, one with 0 < j_eff < J, one with j_eff = J and, at d < 2 J, one with 2 j_eff > d"""
    seen = set()
    for d, J, regime in W.GRID:
        kp = H.kpad_for(J)
        seen |= {"woodbury:%d:%d" % (kp, m) for op in W.OPS for m in W.LAUNCHES[op]} | {"woodbury_diag:%d" % kp}
    assert seen == set(W.plan_names()) and len(seen) == 35
    assert {(H.kpad_for(J), d) for d, J, r in W.GRID if r == "plain"} == {(kp, d) for kp in W.KPADS for d in W.grid_dims(kp)}
    assert {(H.kpad_for(J), r) for _, J, r in W.GRID if r != "plain"} == {(kp, r) for kp in (12, 32) for r in ("scaled", "dep")}
    assert len({W.case_id(c) for c in W.GRID}) == len(W.GRID)
    for case in W.GRID:
        c = W.grid_case(case)
        th, gr, walks = fr.oracle_walk(c)
        jeff = [int(walks[k][1][l]) for k, l in W.grid_points(case, c.lengths)]
        for what, pred in W.grid_needs(case).items():
            assert any(pred(j) for j in jeff), (W.case_id(case), what, jeff)
