"""The teacher-forced L-BFGS step checker (tests/lbfgs_step_reference.py) on the CPU, before any GPU time is spent:

  * it PASSES on both fp64 CPU implementations of this repository's L-BFGS -- pfmi.optimize.optimize_with_trace (NumPy two-loop
    recursion; also with its `_reject_every` hook) and the oracle's scalar C driver po.optimize_trace -- on the whole case grid of
    tests/test_gpu_lbfgs_steps.py at the same starting points, within the exemption cap, and every case meets the coverage condition
    the GPU test asserts (ring wrapped for at least 4 steps; a full turn where J <= 6);
  * it CATCHES a wrong implementation: `variant=` alters the reference, which is the same as checking a wrong kernel against the right
    reference, and every variant fails assertion (a) or (b) -- the eviction and slot variants only once the ring is wrapped / full;
  * the grid reaches every instantiation pf_launch_lbfgs can dispatch to.
"""
import numpy as np
import pytest

from helpers import oracle_target
from oracle import pf_oracle as po
import lbfgs_step_reference as R

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)

ALL = R.GRID + R.CLOSURE_GRID
_CASES = {c[0]: c for c in ALL}
_TRACES = {}


def _host_trace(pfmi_mod, cid, k=0):
    """the host twin's trace of path k of a grid case (computed once, shared, never modified)"""
    from pfmi.optimize import optimize_with_trace
    if (cid, k) not in _TRACES:
        _, tn, d, J, maxit, rej, sc = _CASES[cid]
        tg = R.grid_target(pfmi_mod, tn, d)
        tr = optimize_with_trace(tg, R.grid_x0(pfmi_mod, d, sc)[k], J, maxit, g_tol=R.G_TOL, _reject_every=rej)
        for a in (tr.points, tr.log_densities, tr.gradients):
            a.setflags(write=False)
        _TRACES[(cid, k)] = (tg, tr)
    return _TRACES[(cid, k)]


@pytest.mark.parametrize("cid", [c[0] for c in ALL])
def test_checker_passes_on_the_host_twin(pfmi_mod, cid):
    """pfmi/optimize.py (with `_reject_every=3` on the grid's hook cases): every step within (a) and (b), no exemption needed beyond the
    cap, stop rule named, coverage condition of the GPU grid met"""
    _, tn, d, J, maxit, rej, sc = _CASES[cid]
    for k in range(R.GRID_K):
        tg, tr = _host_trace(pfmi_mod, cid, k)
        recs, s = R.check_trace(tr.points, tr.log_densities, tr.gradients, J, maxit, R.G_TOL, fg=tg.logp_and_grad, reject_every=rej)
        print(cid, k, {q: s[q] for q in ("steps", "max_h", "wrapped", "turns", "rejected", "restarts", "exempt", "borderline", "max_ratio_a",
                                         "max_ratio_b", "stop")})
        R.assert_trace(cid, recs, s, J, impl="host twin")
        assert R.coverage_ok(s, J), (cid, k, s["wrapped"], s["turns"], s["steps"])
        assert s["max_h"] == J
        if rej:
            assert s["rejected"] >= s["steps"] // rej


@pytest.mark.parametrize("cid", [c[0] for c in ALL if not c[5]])
def test_checker_passes_on_the_oracle_driver(pfmi_mod, cid):
    """oracle/pf_oracle.c: pfo_optimize_trace (scalar C, every sum left to right; it has no reject hook)"""
    _, tn, d, J, maxit, rej, sc = _CASES[cid]
    tg = R.grid_target(pfmi_mod, tn, d)
    x0 = R.grid_x0(pfmi_mod, d, sc)
    for k in range(R.GRID_K):
        P, L, G = po.optimize_trace(oracle_target(tg), x0[k], J, maxit, R.G_TOL)
        recs, s = R.check_trace(P, L, G, J, maxit, R.G_TOL, fg=tg.logp_and_grad)
        print(cid, k, {q: s[q] for q in ("steps", "max_h", "wrapped", "turns", "rejected", "restarts", "exempt", "borderline", "max_ratio_a",
                                         "max_ratio_b", "stop")})
        R.assert_trace(cid, recs, s, J, impl="oracle driver")
        assert R.coverage_ok(s, J), (cid, k, s["wrapped"], s["turns"], s["steps"])


def test_checker_without_fg_uses_wolfe_and_dyadic_step(pfmi_mod):
    """fg=None: (b) is strong Wolfe from the recorded values plus a dyadic a_fit / a0"""
    cid = "w64-lr8-J6"
    tg, tr = _host_trace(pfmi_mod, cid)
    J, maxit = _CASES[cid][3], _CASES[cid][4]
    recs, s = R.check_trace(tr.points, tr.log_densities, tr.gradients, J, maxit, R.G_TOL)
    assert not s["failures"] and s["stop"] == "converged"
    recs, s = R.check_trace(tr.points, tr.log_densities, tr.gradients, J, maxit, R.G_TOL, variant="a0_one")
    assert s["first_failure"][:2] == (0, "b")


# ---- mutations: (variant, case, step of the first failure, why that step) ---------------------------------------------------------------
def _first_failure(pfmi_mod, cid, variant, reject_every=None):
    tg, tr = _host_trace(pfmi_mod, cid)
    _, tn, d, J, maxit, rej, sc = _CASES[cid]
    recs, s = R.check_trace(tr.points, tr.log_densities, tr.gradients, J, maxit, R.G_TOL, fg=tg.logp_and_grad,
                            reject_every=rej if reject_every is None else reject_every, variant=variant)
    return s, recs


@pytest.mark.parametrize("variant,cid,first", [
    ("gamma_one", "w64-lr8-J6", 1),           # step 1 is the first with a pair in the ring
    ("gamma_one", "w512-lr16-J16", 1),
    ("flip_gYt", "w64-lr8-J6", 1),
    ("flip_gYt", "w256g-diag-J10", 1),
    ("gamma_oldest", "w64-lr8-J6", 2),        # step 2 is the first whose oldest pair is not its newest
    ("gamma_oldest", "w512-lr16-J16", 2),
])
def test_mutation_caught_from_the_first_pair_on(pfmi_mod, variant, cid, first):
    s, recs = _first_failure(pfmi_mod, cid, variant)
    assert s["first_failure"] is not None and s["first_failure"][0] == first, s["failures"][:3]
    assert s["first_failure"][1] == "a"


@pytest.mark.parametrize("cid", ["w64-lr8-J6", "w256g-diag-J10", "w512-lr16-J16"])
def test_mutation_ring_of_J_minus_1_fails_only_once_the_ring_is_full(pfmi_mod, cid):
    """a ring that holds J - 1 pairs gives the right direction up to step J - 1 (J - 1 pairs) and the wrong one at step J, the first
    step whose ring is full"""
    J = _CASES[cid][3]
    ok, _ = _first_failure(pfmi_mod, cid, None)
    s, recs = _first_failure(pfmi_mod, cid, "ring_Jm1")
    assert ok["first_full"] == J and s["first_failure"][:2] == (J, "a"), (ok["first_full"], s["failures"][:3])


@pytest.mark.parametrize("cid", ["w64-lr8-J6", "w256g-diag-J10", "w512-lr16-J16"])
def test_mutation_evict_newest_fails_only_once_the_ring_has_wrapped(pfmi_mod, cid):
    """the first eviction happens behind step J; step J + 1 is the first with head != 0 and the first to fail"""
    J = _CASES[cid][3]
    ok, _ = _first_failure(pfmi_mod, cid, None)
    s, recs = _first_failure(pfmi_mod, cid, "evict_newest")
    assert ok["first_wrapped"] == J + 1 and s["first_failure"][:2] == (J + 1, "a"), (ok["first_wrapped"], s["failures"][:3])


@pytest.mark.parametrize("variant,cid,fails", [
    ("skip_slot_6", "w256g-diag-J10", True), ("skip_slot_6", "w512-lr16-J16", True), ("skip_slot_6", "w64-lr8-J6", False),
    ("skip_slot_4", "clo-lr8-J6", True), ("skip_slot_4", "w256g-diag-J10", True), ("skip_slot_4", "clo-lr8-J24", False),
    ("skip_slot_2", "w64-diag-J1", True), ("skip_slot_2", "w512-diag-J2", False),
])
def test_mutation_skipped_slot_of_a_ragged_batch_fails_only_once_the_ring_is_full(pfmi_mod, variant, cid, fails):
    """slot J - 1 left out of the full ring when J is no multiple of the batch (6: built-in kernel up to 256 threads, 2: 512 threads,
    4: closure kernel): step J, the first with a full ring, is the first to fail; a J that is a multiple of the batch has no ragged
    batch and the variant changes nothing"""
    J = _CASES[cid][3]
    s, recs = _first_failure(pfmi_mod, cid, variant)
    if fails:
        assert s["first_failure"][:2] == (J, "a"), s["failures"][:3]
    else:
        assert not s["failures"]


@pytest.mark.parametrize("cid", ["w64-lr8-J6", "w256g-diag-J10", "w512x-diag-J6"])
def test_mutation_a0_one_after_restart_fails_the_step_length_at_step_0(pfmi_mod, cid):
    """the first step starts from an empty ring, a0 = 1 / |g|_2 < 1: with a0 = 1 the replayed search ends elsewhere; the direction -g is
    untouched, so only (b) fails, and only there"""
    s, recs = _first_failure(pfmi_mod, cid, "a0_one")
    assert s["failures"] and all(f[:2] == (0, "b") for f in s["failures"]), s["failures"][:3]
    assert recs[0]["a0"] == 1.0 and recs[0]["a_fit"] < 1.0


@pytest.mark.parametrize("cid,made_with,checked_with", [("w64-lr8-J6-rej", 3, 0), ("w512-diag-J6-rej", 3, 0), ("w64-lr8-J6", 0, 3)])
def test_reject_hook_mismatch_is_caught(pfmi_mod, cid, made_with, checked_with):
    """the pair of step 2 (the third) is dropped by one side only: step 3 is the first whose rings differ"""
    assert _CASES[cid][5] == made_with
    s, recs = _first_failure(pfmi_mod, cid, None, reject_every=checked_with)
    assert s["first_failure"][:2] == (3, "a"), s["failures"][:3]


def test_stop_rules_are_named_and_a_late_stop_is_caught(pfmi_mod):
    """(d): a converged trace; the same trace cut short (no stop reason); the same trace with a point behind the converged one"""
    cid = "w64-lr8-J6"
    tg, tr = _host_trace(pfmi_mod, cid)
    J, maxit = _CASES[cid][3], _CASES[cid][4]
    P, L, G = tr.points, tr.log_densities, tr.gradients
    assert R.check_trace(P, L, G, J, maxit, R.G_TOL)[1]["stop"] == "converged"
    s = R.check_trace(P[:-3], L[:-3], G[:-3], J, maxit, R.G_TOL)[1]
    assert s["stop"] == "none"
    assert R.check_trace(P[:31], L[:31], G[:31], J, 30, R.G_TOL)[1]["stop"] == "maxiters"
    late = R.check_trace(np.vstack([P, P[-1:]]), np.r_[L, L[-1]], np.vstack([G, G[-1:]]), J, maxit, R.G_TOL)[1]
    assert late["early_stop_points"] == [len(P) - 1]
    bad = G.copy()
    bad[-1, 3] = np.nan
    assert R.check_trace(P, L, bad, J, maxit, R.G_TOL)[1]["stop"] == "non-finite"
    still = R.check_trace(np.vstack([P[:10], P[9:10]]), np.r_[L[:10], L[9]], np.vstack([G[:10], G[9:10]]), J, maxit, R.G_TOL)[1]
    assert still["stop"] == "not moved"


# ---- the grid reaches every instantiation ----------------------------------------------------------------------------------------------
def _dispatch(d, J, r, funnel):
    """pf_launch_lbfgs (csrc/lbfgs_kernels.hip) restated: threads, elements per thread, padded target rank, ring in LDS"""
    nt = 64 if d <= 256 else 256 if d <= 1024 else 512
    ept = 4 if d <= 1024 else 20 if d <= 10240 else 32
    hist_bytes = 8 * 2 * J * nt * ept
    gram_bytes = 8 * (nt // 64) * (2 * J * J + 3 * J)
    lds = hist_bytes + gram_bytes <= 140 * 1024
    rpad = 0 if (funnel or r == 0) else 8 if r <= 8 else 16             # api_inputs.hip: T.rpad; the funnel takes the RPAD 0 instance
    return ept, nt, rpad, lds


def test_grid_reaches_every_lbfgs_instantiation():
    want = {(e, n, rp, lds) for (e, n, lds) in [(4, 64, True), (4, 256, True), (4, 256, False), (20, 512, False), (32, 512, False)]
            for rp in (0, 8, 16)}
    got, funnel_shapes, ragged = set(), set(), set()
    for cid, tn, d, J, maxit, rej, sc in R.GRID:
        assert maxit <= 120 and d <= 16384 and 1 <= J <= 16
        r = 0 if tn in ("diag", "funnel") else int(tn[2:])
        inst = _dispatch(d, J, r, tn == "funnel")
        if tn == "funnel":
            funnel_shapes.add(inst[:2])
        else:
            got.add(inst)
        ch = 6 if inst[1] <= 256 else 2
        if J % ch:
            ragged.add((inst[1], inst[3], J % ch))
    assert got == want, (sorted(want - got), sorted(got - want))
    assert len(want) == 15
    assert funnel_shapes == {(4, 64), (4, 256)}
    # unreachable: a ring in LDS at 512 threads (J = 1 needs 160 KiB) and a global ring at 64 threads (J = 16 needs 73 KiB)
    assert not _dispatch(1025, 1, 0, False)[3] and _dispatch(256, 16, 0, False)[3]
    # ragged last batches of the fused reduction: 6 slots at up to 256 threads (J = 1, 10, 16 -> 1, 4, 4 live slots)
    assert {(64, True, 1), (64, True, 4), (256, False, 4)} <= ragged
    # one reject-hook case per workgroup shape (and ring placement at 256 threads); the closure kernel: J = 6, 24, 32 at d = 50, d = 20 000
    hooked = {_dispatch(d, J, 0, False)[:2] + (_dispatch(d, J, 0, False)[3],) for cid, tn, d, J, maxit, rej, sc in R.GRID if rej}
    assert hooked == {(4, 64, True), (4, 256, True), (4, 256, False), (20, 512, False), (32, 512, False)}
    clo = {(d, J, bool(rej)) for cid, tn, d, J, maxit, rej, sc in R.CLOSURE_GRID}
    assert {(50, 6, False), (50, 24, False), (50, 32, False), (20000, 6, False)} <= clo and any(c[2] for c in clo)
