"""pfmi_pool_transform / pfmi_pool_transform_revert (csrc/pool_transform_kernels.hip) and pfmi.moment_match on the GPU.

The move is checked bit for bit against the correctly rounded a x + b, logp of the moved columns against the long-double reference
evaluated at the GPU's OWN moved columns inside the derived bound (tests/pool_transform_reference.py), the ratios to the last bit of
the stated host sum, the state machine (revert, identity, cumulative trials, a new pool, the error codes) on the buffers a caller can
read, and the loop against its NumPy restatement run on the GPU's own pool as built with the oracle's PSIS."""
import numpy as np
import pytest

import margins as mg
import pool_transform_reference as R
from helpers import demo_device_target, demo_host_target, make_traces
from pool_common import LD, U, run_two_engines

pytestmark = pytest.mark.gpu
J = 6
DS = (1, 3, 63, 64, 65, 127, 128, 130)         # packed columns below 64, lanes along rows from 64, paired loads from even d >= 128
KN = ((1, 1), (1, 25), (3, 257))
_TR = {}


def _fit(pfmi, eng, d, runs):
    """the engine fitted to the traces `runs` (indices into three traces of t_diag(d), three iterations each)"""
    if d not in _TR:
        _TR[d] = make_traces(pfmi.t_diag(d), 3, 11, history_length=J, maxiters=3)
    tr = [_TR[d][k] for k in runs]
    eng.set_target(pfmi.t_diag(d))
    eng.set_traces([t.points for t in tr], [t.gradients for t in tr])
    eng.fit_batch(J)


def _build(eng, tg, runs, N_r):
    """pool of N_r draws of every fitted path's last fit under target `tg` (the fits stay); returns (points, seeds)"""
    eng.set_target(tg)
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(len(runs))]
    seeds = np.array([1000 + 7 * k for k in runs], dtype=np.uint64)
    eng.pool_build(N_r, pts, seeds)
    return pts, seeds


def _as_built(eng, pts, seeds, N_r):
    """(lp0, lq0) of the pool from pfmi_draws, whose blocks are the pool's bit for bit"""
    parts = [eng.draws(p, s, N_r) for p, s in zip(pts, seeds)]
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def _map(d, seed=3):
    rng = np.random.default_rng(seed + d)
    return 0.5 + rng.random(d), rng.normal(size=d)


def _lr_mix(eng):
    ptr, n = eng.pool_mixture_ratios_dev()
    return eng.memcpy_d2h(np.empty(n), ptr)


def _bits(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64), err_msg=what)


# ---- the move and the ratios, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_move_and_ratios_bit_for_bit(pfmi_mod, eng, d):
    pfmi = pfmi_mod
    scale, shift = _map(d)
    sla = R.sum_log_scale(scale)
    for K, N_r in KN:
        runs = list(range(K))
        _fit(pfmi, eng, d, runs)
        pts, seeds = _build(eng, pfmi.t_diag(d), runs, N_r)
        P0, lr0 = eng.pool_get()
        P0 = np.array(P0)
        lp0, lq0 = _as_built(eng, pts, seeds, N_r)
        _bits(lr0, lp0 - lq0, "precondition: the pool's ratios are those of pfmi_draws")
        lmix0, _ = eng.pool_mixture_ratios()
        lp1, lr1 = eng.pool_transform(scale, shift)
        P1, lr1g = eng.pool_get()
        _bits(np.array(P1).reshape(d, -1, order="F"), R.exact_move(scale, shift, P0.reshape(d, -1, order="F")), f"move d={d} K={K} N_r={N_r}")
        _bits(lr1g, lr1)
        lq1, lr1_ref = R.moved_ratios(lp1, lq0, scale)
        _bits(lr1, lr1_ref, "lr' = lp' - (lq0 - sum log scale)")
        _bits(_lr_mix(eng), lp1 - (lmix0 - sla), "lr_mix' = lp' - (lmix0 - sum log scale)")
        # scale alone and shift alone: the NULL forms are ones and zeros
        eng.pool_transform(None, shift, want=False)
        _bits(np.array(eng.pool_get()[0]).reshape(d, -1, order="F"), R.exact_move(np.ones(d), shift, P0.reshape(d, -1, order="F")))
        lp_s, lr_s = eng.pool_transform(scale, None)
        _bits(np.array(eng.pool_get()[0]).reshape(d, -1, order="F"), R.exact_move(scale, np.zeros(d), P0.reshape(d, -1, order="F")))
        _bits(lr_s, lp_s - lq1)


# ---- logp of the moved columns ----------------------------------------------------------------------------------------------------------
def _families(pfmi, d):
    out = [("r0", pfmi.t_diag(d, seed=3)), ("funnel", pfmi.t_funnel(d))]
    out += [(f"r{r}", pfmi.t_lowrank(d, r=r, seed=2, wscale=2 / np.sqrt(d))) for r in (3, 8, 16) if d >= r]
    return out


def _check_logp(pfmi, eng, d, tg, name, runs, N_r):
    _build(eng, tg, runs, N_r)
    scale, shift = _map(d, seed=5)
    lp1, _ = eng.pool_transform(scale, shift)
    X1 = np.array(eng.pool_get()[0]).reshape(d, -1, order="F")
    ref, bound = R.ref_logp(tg, X1)
    ratio = np.abs(lp1.astype(LD) - ref) / bound
    print(f"pool_transform logp d={d} {name}: worst |gpu - ref| / bound = {float(ratio.max()):.3g}")
    mg.check("pool_transform", f"logp_bound@{name}", float(ratio.max()), bound=1.0, contract=1.0, ctx=f"d={d}")


@pytest.mark.parametrize("d", DS)
def test_logp_of_the_moved_columns_inside_the_derived_bound(pfmi_mod, eng, d):
    runs = [0, 1, 2]
    _fit(pfmi_mod, eng, d, runs)
    for name, tg in _families(pfmi_mod, d):
        _check_logp(pfmi_mod, eng, d, tg, name, runs, 257)


def test_logp_at_d_1000(pfmi_mod, eng):
    _fit(pfmi_mod, eng, 1000, [0, 1])
    _check_logp(pfmi_mod, eng, 1000, pfmi_mod.t_lowrank(1000, r=8, seed=2, wscale=2 / np.sqrt(1000)), "r8", [0, 1], 64)


def test_host_and_device_closures_see_the_moved_pool(pfmi_mod, eng):
    """a closure target's pool is drawn by the draw kernel that materialises x for the closure, whose columns may differ from the
    built-in route's in the last bit (the draws contract), so each route's move is checked against ITS OWN pool as built and the
    closures' logp' against the built-in route's within the logp contract"""
    pfmi, d = pfmi_mod, 65
    tg = pfmi.t_lowrank(d, r=3, seed=2, wscale=2 / np.sqrt(d))
    scale, shift = _map(d, seed=9)
    _fit(pfmi, eng, d, [0, 1, 2])
    out = {}
    for name, t in (("builtin", tg), ("host", demo_host_target(tg)), ("device", demo_device_target(tg))):
        _build(eng, t, [0, 1, 2], 257)
        P0 = np.array(eng.pool_get()[0]).reshape(d, -1, order="F")
        lp, lr = eng.pool_transform(scale, shift)
        P1 = np.array(eng.pool_get()[0]).reshape(d, -1, order="F")
        _bits(P1, R.exact_move(scale, shift, P0), f"{name}: the move")
        out[name] = (lp, lr, P0)
    for name in ("host", "device"):
        mg.check("pool_transform", f"draws@{name}_closure", np.max(np.abs(out[name][2] - out["builtin"][2]) / (1 + np.abs(out["builtin"][2]))))
        mg.check("pool_transform", f"logp@{name}_closure", mg.rel(out[name][0], out["builtin"][0]))
        mg.check("pool_transform", f"logp@{name}_closure_ratio", mg.rel(out[name][1], out["builtin"][1]))


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def _state(eng, mix):
    P, lr = eng.pool_get()
    return [np.array(P), lr] + ([_lr_mix(eng)] if mix else [])


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        _bits(x, y, what)


@pytest.mark.parametrize("d", (3, 130))
def test_state_machine(pfmi_mod, eng, d):
    pfmi = pfmi_mod
    tg = pfmi.t_diag(d, seed=3)
    A, B = _map(d, seed=1), _map(d, seed=2)
    runs, N_r = [0, 1, 2], 257
    _fit(pfmi, eng, d, runs)
    pts, seeds = _build(eng, tg, runs, N_r)
    lp0, lq0 = _as_built(eng, pts, seeds, N_r)
    eng.pool_mixture_ratios(want=False)
    built = _state(eng, True)
    eng.psis(built[1])
    w0 = eng.psis_weights(len(lp0))
    # one trial, undone: every buffer back, a second revert refused
    lpA, _ = eng.pool_transform(*A)
    moved_A = _state(eng, True)
    assert not np.array_equal(moved_A[0], built[0])
    eng.pool_transform_revert()
    _same(_state(eng, True), built, "revert after the first trial")
    with pytest.raises(pfmi.PfmiError) as ex:
        eng.pool_transform_revert()
    assert ex.value.code == -3
    # two different trials in a row: each equals itself applied alone (cumulative from the pool as built, not stacked)
    eng.pool_transform(*A, want=False)
    lpB, _ = eng.pool_transform(*B)
    after_AB = _state(eng, True)
    eng.pool_transform_revert()                                     # the state before B is A's
    _same(_state(eng, True), moved_A, "revert after the second trial")
    lpA2, _ = eng.pool_transform(*A)                                # A over A: the same bits again
    _bits(lpA2, lpA)
    _build(eng, tg, runs, N_r)                                      # a new pool clears the state
    with pytest.raises(pfmi.PfmiError) as ex:
        eng.pool_transform_revert()
    assert ex.value.code == -3
    _same(_state(eng, False), built[:2], "a new pool is the pool as built")
    eng.pool_mixture_ratios(want=False)
    lpB1, _ = eng.pool_transform(*B)
    _same(_state(eng, True), after_AB, "B alone equals B after A")
    _bits(lpB1, lpB)
    # the identity call: the pool as built, without a pass; its revert puts the moved pool back
    lpI, lrI = eng.pool_transform(None, None)
    _same(_state(eng, True), built, "identity")
    _bits(lpI, lp0)
    _bits(lrI, lp0 - lq0)
    eng.pool_transform_revert()
    _same(_state(eng, True), after_AB, "revert of the identity call")
    eng.pool_transform(None, None, want=False)
    eng.pool_transform(None, None, want=False)                      # identity over the pool as built: nothing moves, one revert allowed
    eng.pool_transform_revert()
    _same(_state(eng, True), built, "identity over the pool as built")
    # the ctx's PSIS weights were never touched
    w1 = eng.psis_weights(len(lp0))
    _bits(w1[0], w0[0])
    _bits(w1[1], w0[1])
    # while the pool is moved its mixture ratios are not recomputed
    eng.pool_transform(*A, want=False)
    with pytest.raises(pfmi.PfmiError) as ex:
        eng.pool_mixture_ratios()
    assert ex.value.code == -3
    _same(_state(eng, True), moved_A, "a refused call leaves the moved pool")


@pytest.mark.parametrize("d", (3, 65, 130))
def test_a_run_does_not_depend_on_k_or_its_position(pfmi_mod, eng, d):
    pfmi = pfmi_mod
    tg = pfmi.t_lowrank(d, r=3, seed=2, wscale=2 / np.sqrt(d))
    scale, shift = _map(d, seed=4)
    N_r = 37
    _fit(pfmi, eng, d, [0, 1, 2])
    _build(eng, tg, [0, 1, 2], N_r)
    lp3, lr3 = eng.pool_transform(scale, shift)
    P3 = np.array(eng.pool_get()[0])
    _fit(pfmi, eng, d, [2])
    _build(eng, tg, [2], N_r)
    lp1, lr1 = eng.pool_transform(scale, shift)
    P1 = np.array(eng.pool_get()[0])
    _bits(P1[:, :, 0], P3[:, :, 2])
    _bits(lp1, lp3[2 * N_r:])
    _bits(lr1, lr3[2 * N_r:])


def test_error_codes_leave_the_pool_intact(pfmi_mod):
    pfmi, d = pfmi_mod, 3
    e = pfmi.Engine(0)
    try:
        _fit(pfmi, e, d, [0, 1])
        e.set_target(pfmi.t_diag(d, seed=3))
        e.N_r = 5
        for call in (lambda: e.pool_transform(np.ones(d), np.zeros(d)), e.pool_transform_revert):      # no pool
            with pytest.raises(pfmi.PfmiError) as ex:
                call()
            assert ex.value.code == -3
        _build(e, pfmi.t_diag(d, seed=3), [0, 1], 5)
        with pytest.raises(pfmi.PfmiError) as ex:                   # nothing to undo
            e.pool_transform_revert()
        assert ex.value.code == -3
        before = _state(e, False)
        ok_s, ok_h = np.array([1.0, 2.0, 0.5]), np.array([0.0, 1.0, -1.0])
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            s = ok_s.copy()
            s[1] = bad
            with pytest.raises(pfmi.PfmiError) as ex:
                e.pool_transform(s, ok_h)
            assert ex.value.code == -1, bad
            _same(_state(e, False), before, f"scale {bad}")
        for bad in (np.nan, np.inf, -np.inf):
            h = ok_h.copy()
            h[2] = bad
            with pytest.raises(pfmi.PfmiError) as ex:
                e.pool_transform(ok_s, h)
            assert ex.value.code == -1, bad
            _same(_state(e, False), before, f"shift {bad}")
        with pytest.raises(pfmi.PfmiError) as ex:                   # a refused call is nothing to undo either
            e.pool_transform_revert()
        assert ex.value.code == -3
        # a refused call changes nothing, what a revert would undo included: the revert after it undoes the last call that succeeded
        e.pool_transform(ok_s, ok_h, want=False)
        moved = _state(e, False)
        with pytest.raises(pfmi.PfmiError) as ex:
            e.pool_transform(-ok_s, ok_h)
        assert ex.value.code == -1
        _same(_state(e, False), moved, "a refused call leaves the moved pool")
        e.pool_transform_revert()
        _same(_state(e, False), before, "the revert after a refused call")
        # a pool of another size after a transform (the spare sets are freed and made again): the move is still the exact one
        e.pool_transform(ok_s, ok_h, want=False)
        _build(e, pfmi.t_diag(d, seed=3), [0, 1], 7)
        with pytest.raises(pfmi.PfmiError) as ex:
            e.pool_transform_revert()
        assert ex.value.code == -3
        P7 = np.array(e.pool_get()[0]).reshape(d, -1, order="F")
        e.pool_transform(ok_s, ok_h, want=False)
        _bits(np.array(e.pool_get()[0]).reshape(d, -1, order="F"), R.exact_move(ok_s, ok_h, P7))
        e.pool_transform_revert()
        _bits(np.array(e.pool_get()[0]).reshape(d, -1, order="F"), P7)
        with pytest.raises(ValueError):
            e.pool_transform(np.ones(d + 1), None)
        e.profile(True)
        e.pool_transform(ok_s, ok_h, want=False)
        ms, n = e.kernel_time("pool_transform")
        assert n == 1 and ms > 0.0 and e.kernel_time("pool_transform_ratio")[1] == 1
        e.profile(False)
    finally:
        e.close()


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def _reference_loop(pfmi, eng, res, mixture):
    """the NumPy loop on the GPU's own pool as built (and its own lq0 / log qbar0), the oracle's target and PSIS"""
    from oracle import pf_oracle as po
    runs = res.pathfinder_results
    pts = [r.fit_distribution.point for r in runs]
    seeds = np.array([r.draw_seed for r in runs], dtype=np.uint64)
    eng.pool_build(R.SC_NR, pts, seeds)
    X0 = np.array(eng.pool_get()[0]).reshape(R.SC_D, -1, order="F")
    lq0 = eng.pool_mixture_ratios()[0] if mixture else _as_built(eng, pts, seeds, R.SC_NR)[1]
    return R.mm_loop(X0, lq0, R.scenario_logp(pfmi), po.psis, k_threshold=R.SC_K_THRESHOLD)


def _check_loop(tag, mr, ref):
    assert [(s, a) for s, _, a in mr.moment_match_history] == [(s, a) for s, _, a in ref["history"]], (mr.moment_match_history, ref["history"])
    assert min(R.history_gaps(ref["history"])) > 1e-6               # (the decisions are clear in the reference: parity of them is a fair demand)
    dk = [abs(a[1] - b[1]) for a, b in zip(mr.moment_match_history, ref["history"])]
    mg.check("moment_match", f"pareto_k@{tag}", max(dk))
    for got, want in ((mr.pool_transform[0], ref["scale"]), (mr.pool_transform[1], ref["shift"])):
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-12, (tag, got, want)
    ks = [k for _, k, a in mr.moment_match_history if a]
    assert all(b < a for a, b in zip(ks, ks[1:])) and ks[0] > 0.7 and ks[-1] < 0.5
    assert mr.psis_result.pareto_shape == ks[-1]
    assert mr.draws.shape == (R.SC_D, 50) and mr.draw_component_ids.min() >= 1 and mr.draw_component_ids.max() <= R.SC_K


@pytest.mark.parametrize("proposal", ("component", "mixture"))
def test_moment_match_follows_the_numpy_loop(pfmi_mod, proposal):
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        res = R.scenario_result(pfmi, [e], proposal)
        ref = _reference_loop(pfmi, e, res, proposal == "mixture")
        mr = res.moment_match(k_threshold=R.SC_K_THRESHOLD)
        _check_loop(proposal, mr, ref)
        assert res.pool_transform is None and mr.proposal == proposal
        dflt = pfmi.moment_match(res)                               # the default threshold stops at the first k-hat <= 0.7
        assert dflt.moment_match_history[-1][1] <= 0.7 and len(dflt.moment_match_history) < len(mr.moment_match_history)
    finally:
        e.close()


_TWO = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/pathfinder.jl_amd"); sys.path.insert(0, sys.argv[1] + "/tests")
import pfmi
import pool_transform_reference as R
out = []
for engs in ([pfmi.Engine(0)], [pfmi.Engine(0), pfmi.Engine(0)]):
    res = R.scenario_result(pfmi, engs)
    mr = res.moment_match(k_threshold=R.SC_K_THRESHOLD)
    out.append((mr, mr.summary(), mr.quantiles(), mr.covariance().cov))
(a, sa, qa, ca), (b, sb, qb, cb) = out
assert len({id(r.fit_distribution.engine) for r in b.pathfinder_results}) == 2
assert a.moment_match_history == b.moment_match_history and len(a.moment_match_history) > 3, (a.moment_match_history, b.moment_match_history)
for x, y in ((a.pool_transform[0], b.pool_transform[0]), (a.pool_transform[1], b.pool_transform[1]), (a.draws, b.draws),
             (a.draw_component_ids, b.draw_component_ids), (a.psis_result.weights, b.psis_result.weights),
             (a.psis_result.log_weights, b.psis_result.log_weights), (sa.mean, sb.mean), (sa.var, sb.var), (qa, qb), (ca, cb)):
    assert np.array_equal(x, y), (x, y)
assert a.psis_result.pareto_shape == b.psis_result.pareto_shape and sa.ess == sb.ess
print("moment_match engines ok", a.psis_result.pareto_shape)
"""


@pytest.mark.timeout(600)
def test_moment_match_over_two_engines_is_bit_identical():
    run_two_engines(_TWO, "moment_match engines ok")


def _check_run_diagnostics(tag, eng, rd, lr, N_r):
    """RunDiagnostics against the downloaded log ratios of the pool it was formed on, run by run: k-hat against the oracle's PSIS of
    the slice; ess and log_evidence with the margins of tests/test_gpu_pool_psis_runs.py (1 / ess within 2 N_r 2^-52 relative of
    np.sum(w^2) of pfmi_psis on the slice; log_evidence = lse - log N_r with lse the constant the route subtracted, read off the
    entries PSIS left alone)"""
    import pool_psis_runs_reference as rr
    import psis_reference as pr
    from oracle import pf_oracle as po
    K = len(lr) // N_r
    assert rd.pareto_shape.shape == rd.ess.shape == rd.log_evidence.shape == (K,) and rd.ndraws_per_run == N_r
    for k in range(K):
        sl = lr[k * N_r:(k + 1) * N_r]
        mg.check("moment_match", f"pareto_k@run_{tag}", abs(rd.pareto_shape[k] - po.psis(sl)[2]))
        ref = eng.psis(sl)
        sumsq = np.sum(ref["weights"] ** 2)
        assert abs(1.0 / rd.ess[k] - sumsq) <= 2 * rr.sumsq_rel_bound(N_r) * sumsq, (tag, k, rd.ess[k], 1.0 / sumsq)
        lw = ref["log_weights"]
        keep = np.setdiff1d(np.arange(N_r), pr.tail_indices(sl)[0])
        lev = sl[keep] - lw[keep] - np.log(float(N_r))
        slack = 2.0 ** -52 * (np.abs(lw[keep]) + 2 * np.abs(sl[keep] - lw[keep]) + 2 * np.abs(lev) + np.log(float(N_r)))
        assert np.all(np.abs(lev - rd.log_evidence[k]) <= slack), (tag, k, np.max(np.abs(lev - rd.log_evidence[k]) / slack))


@pytest.mark.parametrize("proposal", ("component", "mixture"))
def test_run_diagnostics_under_the_mixture_on_a_matched_result(pfmi_mod, proposal):
    """run_diagnostics(source="mixture") of a matched result: the mixture ratios are formed on the pool as built and carried along by
    the result's map, so the call equals per-run PSIS of the downloaded lr_mix' -- for a result matched under the mixture proposal and
    for one matched under the per-run proposals alike"""
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        res = R.scenario_result(pfmi, [e], proposal)
        mr = res.moment_match(k_threshold=R.SC_K_THRESHOLD)
        assert mr.pool_transform is not None
        rd = mr.run_diagnostics(source="mixture")
        P1 = np.array(e.pool_get()[0]).reshape(R.SC_D, -1, order="F")
        lrm = _lr_mix(e)
        X0 = np.concatenate([e.draws(r.fit_distribution.point, r.draw_seed, R.SC_NR)[0] for r in res.pathfinder_results], axis=1)
        _bits(P1, R.exact_move(mr.pool_transform[0], mr.pool_transform[1], X0), "the diagnostics ran on the matched pool")
        _check_run_diagnostics(f"mixture_{proposal}", e, rd, lrm, R.SC_NR)
        plain = res.run_diagnostics(source="mixture")                 # the unmatched result: the other pool, other numbers
        assert not np.array_equal(plain.pareto_shape, rd.pareto_shape)
    finally:
        e.close()


# ---- carry-over -------------------------------------------------------------------------------------------------------------------------
def test_matched_result_carries_its_move_and_the_unmatched_one_is_untouched(pfmi_mod):
    from pool_cross_reference import covariance
    from pool_quantiles_reference import quantiles
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        res = R.scenario_result(pfmi, [e])
        probs = (0.025, 0.25, 0.5, 0.75, 0.975)
        before = (res.summary(), res.quantiles(probs), res.covariance(), res.run_diagnostics())
        mr = res.moment_match(k_threshold=R.SC_K_THRESHOLD)
        after = (res.summary(), res.quantiles(probs), res.covariance(), res.run_diagnostics())
        for f in ("mean", "var", "std", "mcse_mean", "run_weights"):
            _bits(getattr(after[0], f), getattr(before[0], f), f"unmatched summary.{f}")
        assert after[0].ess == before[0].ess and after[0].pareto_shape == before[0].pareto_shape
        _bits(after[1], before[1], "unmatched quantiles")
        _bits(after[2].cov, before[2].cov, "unmatched covariance")
        for f in ("pareto_shape", "ess", "log_evidence"):
            _bits(getattr(after[3], f), getattr(before[3], f), f"unmatched run_diagnostics.{f}")
        # the matched result: every summary from the matched pool and its weights, downloaded after the call that rebuilt them
        s = mr.summary()
        P = np.array(e.pool_get()[0])
        lr = e.pool_get(draws=False)[1]
        S = R.SC_K * R.SC_NR
        w = e.psis_weights(S)[0]
        _bits(w, mr.psis_result.weights, "the rebuilt matched pool has the matched result's weights")
        P2 = P.reshape(R.SC_D, -1, order="F")
        _bits(P2, R.exact_move(mr.pool_transform[0], mr.pool_transform[1],
                               np.concatenate([e.draws(r.fit_distribution.point, r.draw_seed, R.SC_NR)[0] for r in res.pathfinder_results], axis=1)),
              "the matched pool is the moved stored draws")
        assert s.pareto_shape == mr.psis_result.pareto_shape and s.ncandidates == S
        mean = np.average(P2, axis=1, weights=w)
        np.testing.assert_allclose(s.mean, mean, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(s.var, np.average((P2 - mean[:, None]) ** 2, axis=1, weights=w), rtol=1e-11)
        assert not np.allclose(s.mean, before[0].mean, rtol=1e-3)
        q = mr.quantiles(probs)
        W = pfmi.api._combine_moments([e.pool_moments(0, True, None)[0]])[0]
        ref, margin = quantiles(P2, w, probs, W)
        safe = margin > 2 * (S + 5) * U * LD(W)
        assert safe.all()
        _bits(q[safe], ref[safe], "matched quantiles")
        c = mr.covariance()
        cref = covariance(P, w)
        ratio = float(np.max(np.abs(c.cov.astype(LD) - cref["cov"]) / (2 * (S + 6) * U * cref["A"] / cref["W"])))
        mg.check("moment_match", "cov", ratio, bound=1.0, contract=1.0)
        rd = mr.run_diagnostics()
        _bits(e.pool_get(draws=False)[1], lr, "run_diagnostics rebuilt the same matched pool")
        _check_run_diagnostics("component", e, rd, lr, R.SC_NR)
        # resample() of the matched result draws from the matched pool
        rs = pfmi.resample(mr, 40)
        assert rs.pool_transform is mr.pool_transform and rs.psis_result is mr.psis_result
        cols = {tuple(c) for c in P2.T}
        assert all(tuple(c) in cols for c in rs.draws.T)
    finally:
        e.close()
