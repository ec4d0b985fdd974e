"""Windowed metric adaptation of the device warm-up (include/pfmi.h: pfmi_chain_scale_set, pfmi_hmc_adapt_metric_enqueue,
pfmi_nuts_adapt_metric_enqueue; the metric kernels of csrc/hmc_metric_kernel.hip and csrc/nuts_metric_kernel.hip).  As in
tests/test_gpu_adapt.py the main check needs no new trajectory checker: a run must be BIT-IDENTICAL to a host-driven replay of its own
step-size and scale traces through the plain calls and pfmi_chain_scale_set.  The replay also gives the state after every warm-up
transition, so the recorded whitened rows, every window's scale and every step-size segment between restarts are checked against the
long-double references of tests/metric_adapt_reference.py, teacher-forced, within the bounds derived there; a plain run on a random scale
passes the step checkers of static HMC and NUTS on ScaledMetric."""
import ctypes as C
import types

import numpy as np
import pytest

import adapt_reference as A
import hmc_reference as H
import metric_adapt_reference as MA
import nuts_reference as N
from helpers import demo_device_target
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON
from test_gpu_adapt import _setup

pytestmark = pytest.mark.gpu

_DONE = {}                         # case -> {"plans", "margins"}: each case runs once


def _route(d, J):
    kpad = H.kpad_for(J)
    return kpad, "res" if H.resident(d, kpad) else "stream"


def _rows(eng, sampler):
    got = eng.hmc_get()
    if sampler == "nuts":
        got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got


def _wait(eng, sampler):
    eng.hmc_wait() if sampler == "hmc" else eng.nuts_wait()


def _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T, record=True, metric=True):
    param = MA.LF if sampler == "hmc" else MA.DEPTH
    if metric:
        (eng.hmc_adapt_metric_enqueue if sampler == "hmc" else eng.nuts_adapt_metric_enqueue)(pts, x0, seeds, eps0, param, W, T, record_whitened=record)
    else:
        (eng.hmc_adapt_enqueue if sampler == "hmc" else eng.nuts_adapt_enqueue)(pts, x0, seeds, eps0, param, W, T)
    _wait(eng, sampler)
    return _rows(eng, sampler), eng.adapt_get(), (eng.adapt_metric_get() if metric else None)


def _plain(eng, sampler, pts, x0, seeds, eps, T, cont, record_path=False):
    if sampler == "hmc":
        eng.hmc_enqueue(pts, None if cont else x0, seeds, eps, MA.LF, T, cont=cont, record_path=record_path)
    else:
        eng.nuts_enqueue(pts, None if cont else x0, seeds, eps, MA.DEPTH, T, cont=cont, record_path=record_path)
    _wait(eng, sampler)
    return _rows(eng, sampler)


def _replay(eng, sampler, pts, x0, seeds, got, warm, met, W, T, label):
    """the run's own traces through the plain calls: one transition at a time with the recorded step size, the recorded scale of window j
    staged in front of transition ends[j]; then one call of T.  Returns the states after the warm-up transitions (K, W, d)."""
    ends = met["window_ends"].tolist()
    states = np.empty((len(pts), W, x0.shape[0]))
    for t in range(W):
        if t in ends:
            eng.chain_scale_set(met["scale_trace"][:, ends.index(t)])
        one = _plain(eng, sampler, pts, x0, seeds, warm["eps_trace"][:, t], 1, cont=t > 0)
        assert np.array_equal(one["accept_prob"][:, 0], warm["accept_trace"][:, t]), (label, t, one["accept_prob"][:, 0], warm["accept_trace"][:, t])
        assert np.array_equal(one["divergent"][:, 0], warm["divergent"][:, t]), (label, t)
        if sampler == "nuts":
            assert np.array_equal(one["n_leapfrog"][:, 0], warm["n_leapfrog"][:, t]), (label, t)
        else:
            assert np.all(warm["n_leapfrog"][:, t] == MA.LF)
        states[:, t] = one["draws"][:, 0, :].T
    last = _plain(eng, sampler, pts, x0, seeds, warm["step_size"], T, cont=True)
    for q in got:
        assert np.array_equal(last[q], got[q]), (label, q)
    return states


def _case(pfmi_mod, eng, case):
    if case in _DONE:
        return _DONE[case]
    d, J, tn, W, T = case
    kpad, route = _route(d, J)
    out = {"plans": set(), "margins": {}}
    pts, x0, eps0, seeds = _setup(pfmi_mod, eng, case)
    status, jeff, _, _ = eng.fit_status()
    metrics = [H.Metric.from_fit(eng.get_fit(int(p), int(jeff[int(p)]))) for p in pts] if HAVE_LONGDOUBLE else None
    init, _, ends = MA.windows(W)
    for sampler in ("hmc", "nuts"):
        label = (MA.case_id(case), sampler)
        plan = "%s_metric:%d:%s" % (sampler, kpad, route)
        others = ["%s%s:%d:%s" % (sampler, s, kpad, route) for s in ("", "_adapt")]
        before, obefore = eng.kernel_time(plan)[1], [eng.kernel_time(o)[1] for o in others]
        got, warm, met = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T)
        launches = eng.kernel_time(plan)[1] - before
        assert [eng.kernel_time(o)[1] for o in others] == obefore                  # the plain and the _adapt plans' counters are untouched
        if sampler == "hmc":
            assert launches == 1 + (W + T) * MA.LF and eng.hmc_stats() == (launches, launches * H.GRID_K)
        else:
            assert 1 + (W + T) <= launches <= 1 + (W + T) * (2 ** MA.DEPTH - 1)
        out["plans"].add(plan)
        assert met["window_ends"].tolist() == ends and met["scale_trace"].shape == (H.GRID_K, len(ends), d)
        assert met["whitened"].shape == (H.GRID_K, ends[-1] - init, d) and got["draws"].shape == (d, T, H.GRID_K)
        assert np.all(np.isfinite(met["scale_trace"])) and np.all(met["scale_trace"] > 0) and np.all(warm["status"] == 0)
        assert np.array_equal(warm["eps_trace"][:, 0], eps0) and np.all(np.isfinite(warm["eps_trace"])) and np.all(warm["eps_trace"] > 0)
        states = _replay(eng, sampler, pts, x0, seeds, got, warm, met, W, T, label)
        if HAVE_LONGDOUBLE:
            for k in range(H.GRID_K):
                run = {"states": states[k], "whitened": met["whitened"][k], "scale_trace": met["scale_trace"][k], "eps_trace": warm["eps_trace"][k],
                       "accept_trace": warm["accept_trace"][k], "step_size": warm["step_size"][k]}
                m = MA.check_run(metrics[k], kpad, x0[:, k], W, 0.8, run)
                for q, v in m.items():
                    out["margins"][q] = max(out["margins"].get(q, 0.0), v)
    print("METRIC_PARITY gpu", MA.case_id(case), "largest error / bound", out["margins"])
    _DONE[case] = out
    return out


@pytest.mark.parametrize("case", MA.CASES, ids=[MA.case_id(c) for c in MA.CASES])
def test_metric_run_is_bit_identical_to_its_replay_and_matches_the_references(pfmi_mod, eng, case):
    """checks 1 - 4: the replay (rows, traces, NUTS statistics), the whitened rows, the scale of every window, every step-size segment"""
    out = _case(pfmi_mod, eng, case)
    if HAVE_LONGDOUBLE:
        assert sorted(out["margins"]) == ["eps", "scale", "whiten"] and max(out["margins"].values()) <= 1.0, out["margins"]


def test_both_factor_routes_ran(pfmi_mod, eng):
    need = {"%s_metric:%d:%s" % ((s,) + _route(c[0], c[1])) for c in MA.CASES for s in ("hmc", "nuts")}
    assert any(p.endswith(":res") for p in need) and any(p.endswith(":stream") for p in need)
    ran = set().union(*[_case(pfmi_mod, eng, case)["plans"] for case in MA.CASES])
    assert need <= ran, need - ran


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)
@pytest.mark.parametrize("case", [(5, 2, "gauss"), (64, 6, "funnel"), (257, 16, "gauss"), (20000, 6, "gauss")], ids=lambda c: MA.case_id(c + (0, 0)))
def test_plain_run_on_a_random_scale_passes_the_step_checkers(pfmi_mod, eng, case):
    d, J, tn = case
    T = 2 if d > 1000 else H.GRID_T
    kpad, route = _route(d, J)
    pts, x0, eps, seeds = _setup(pfmi_mod, eng, case)
    status, jeff, _, _ = eng.fit_status()
    scale = 0.5 + 1.5 * np.random.default_rng(d + J).random((H.GRID_K, d))
    for sampler in ("hmc", "nuts"):
        plain = _plain(eng, sampler, pts, x0, seeds, eps, T, cont=False)
        eng.chain_scale_set(np.ones((H.GRID_K, d)))
        ones = _plain(eng, sampler, pts, x0, seeds, eps, T, cont=False)
        for q in plain:
            assert np.array_equal(ones[q], plain[q]), (sampler, q)                 # a scale of ones: the bits of the unscaled run
        before = eng.kernel_time("%s_metric:%d:%s" % (sampler, kpad, route))[1]
        eng.chain_scale_set(scale)
        got = _plain(eng, sampler, pts, x0, seeds, eps, T, cont=False, record_path=True)
        assert eng.kernel_time("%s_metric:%d:%s" % (sampler, kpad, route))[1] > before
        path = eng.hmc_path() if sampler == "hmc" else eng.nuts_path()
        stats = (got["tree_depth"], got["n_leapfrog"]) if sampler == "nuts" else None
        borderline = decisions = 0
        for k in range(H.GRID_K):
            p = int(pts[k])
            S = MA.ScaledMetric(H.Metric.from_fit(eng.get_fit(p, int(jeff[p]))), scale[k])
            if sampler == "hmc":
                o = H.check(S, H.gpu_recording(x0[:, k], path, got, k), int(seeds[k]), float(eps[k]), MA.LF, kpad, label=(case, k))
                decisions += T
            else:
                o = N.check(S, N.gpu_recording(x0[:, k], path, got, stats, k), int(seeds[k]), float(eps[k]), MA.DEPTH, kpad, label=(case, k))
                decisions += o["decisions"]
            borderline += o["borderline"]
            print("METRIC_STEP", sampler, MA.case_id(case + (0, 0)), k, {q: float("%.3g" % m) for q, m in o["margins"].items()})
            assert max(o["margins"].values()) <= 1.0
        assert borderline <= (2 * decisions) // 100, (sampler, borderline, decisions)


@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_short_warm_up_is_the_step_size_warm_up(pfmi_mod, eng, sampler):
    case = (64, 6, "gauss", 12, 3)
    pts, x0, eps0, seeds = _setup(pfmi_mod, eng, case)
    plan = "%s_adapt:%d:%s" % ((sampler,) + _route(64, 6))
    a_got, a_warm, _ = _adaptive(eng, sampler, pts, x0, seeds, eps0, 12, 3, metric=False)
    before = eng.kernel_time(plan)[1]
    m_got, m_warm, met = _adaptive(eng, sampler, pts, x0, seeds, eps0, 12, 3, record=False)
    assert eng.kernel_time(plan)[1] > before                                       # today's warm kernels
    for q in a_got:
        assert np.array_equal(a_got[q], m_got[q]), q
    for q in a_warm:
        if q != "status":
            assert np.array_equal(a_warm[q], m_warm[q]), q
    assert np.all(a_warm["status"] == 0) and np.all(m_warm["status"] == MA.NO_METRIC_WINDOW)
    assert len(met["window_ends"]) == 0 and met["scale_trace"].shape == (H.GRID_K, 0, 64)


def test_return_codes_and_forgetting(pfmi_mod):
    from pfmi import _lib
    L = _lib.lib()
    d, K = 12, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
    seeds = np.array([1, 2], dtype=np.uint64)
    i64p, u64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

    def enq(fn, W=25, T=2, flags=0, k=K):
        pts, eps = np.zeros(k, dtype=np.int64), np.full(k, 0.1)
        return fn(e.ctx, k, pts.ctypes.data_as(i64p), x0.ctypes.data_as(dp), seeds.ctypes.data_as(u64p), eps.ctypes.data_as(dp), 2, W, T, 0.8, flags)

    def metric_get():
        return L.pfmi_adapt_metric_get(e.ctx, None, None, None, None)

    def no_chains():
        return L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3

    try:
        with pytest.raises(pfmi_mod.PfmiError):
            e.adapt_metric_get()
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert metric_get() == -3                                                   # PFMI_ERR_STATE: no such run
        for fn, wait in ((L.pfmi_hmc_adapt_metric_enqueue, L.pfmi_hmc_wait), (L.pfmi_nuts_adapt_metric_enqueue, L.pfmi_nuts_wait)):
            for bad in (dict(flags=1), dict(flags=2), dict(flags=8), dict(flags=5), dict(W=0), dict(W=-3)):
                assert enq(fn) == 0 and wait(e.ctx) == 0 and metric_get() == 0
                assert enq(fn, **bad) == -1 and no_chains() and metric_get() == -3, bad          # PFMI_ERR_ARG, and no chains left
            assert enq(fn, flags=MA.RECORD_WHITENED) == 0 and wait(e.ctx) == 0 and metric_get() == 0
            # a scale staged for another K, and a scale value that is not positive and finite
            assert L.pfmi_chain_scale_set(e.ctx, 3, np.ones((3, d)).ctypes.data_as(dp)) == 0
            assert enq(fn) == -1 and no_chains()
            assert enq(fn) == 0 and wait(e.ctx) == 0                                # (the refused call took the staging with it)
            for v in (0.0, -1.0, np.inf, np.nan):
                c = np.ones((K, d))
                c[1, 3] = v
                assert enq(fn) == 0 and wait(e.ctx) == 0
                assert L.pfmi_chain_scale_set(e.ctx, K, c.ctypes.data_as(dp)) == -1 and no_chains(), v
            assert L.pfmi_chain_scale_set(e.ctx, 0, np.ones((K, d)).ctypes.data_as(dp)) == -1
            assert L.pfmi_chain_scale_set(e.ctx, K, None) == 0
        # an adaptive run without metric windows does not serve adapt_metric_get
        e.hmc_adapt_enqueue([0, 0], x0, seeds, [0.1, 0.1], 2, 25, 2)
        e.hmc_wait()
        assert metric_get() == -3 and L.pfmi_adapt_get(e.ctx, None, None, None, None, None, None) == 0
        # a run that did not record its whitened rows has none to give
        e.hmc_adapt_metric_enqueue([0, 0], x0, seeds, [0.1, 0.1], 2, 25, 2)
        e.hmc_wait()
        buf = np.empty((K, 25, d))
        assert L.pfmi_adapt_metric_get(e.ctx, None, None, None, buf.ctypes.data_as(dp)) == -3
        # a new fit forgets the scale, resident and staged: the next fresh run launches the plain kernel
        plain, metric = "hmc:%d:res" % H.kpad_for(6), "hmc_metric:%d:res" % H.kpad_for(6)
        e.chain_scale_set(np.full((K, d), 1.5))
        e.fit_batch(6)
        assert no_chains() and metric_get() == -3
        b_plain, b_metric = e.kernel_time(plain)[1], e.kernel_time(metric)[1]
        e.hmc_enqueue([0, 0], x0, seeds, [0.1, 0.1], 2, 1)
        e.hmc_wait()
        assert e.kernel_time(plain)[1] > b_plain and e.kernel_time(metric)[1] == b_metric
    finally:
        e.close()


@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_chains_sample_the_target_after_the_metric_warm_up(pfmi_mod, eng, sampler):
    """hmc_reference.sampling_case with every chain on the path's first point as its metric, through pfmi.hmc / pfmi.nuts with
    adapt_metric=True (tests/test_metric_adapt_cpu.py admits the case on the mirror)"""
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(demo_device_target(tg, grad=True))
    x = pfmi_mod.HostRNG(5).rand(tg.d).reshape(1, tg.d) * 4 - 2
    eng.optimize_batch(x, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(eng.d)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    result = types.SimpleNamespace(draws=X0, fit_distribution=types.SimpleNamespace(engine=eng, point=0, token=eng.fit_token()))
    fn, kw = (pfmi_mod.hmc, dict(nleapfrog=H.SAMPLING_LF)) if sampler == "hmc" else (pfmi_mod.nuts, dict(max_depth=5))
    out = fn(result, A.SAMPLING_T, nwarmup=A.SAMPLING_W, rng=pfmi_mod.HostRNG(777), adapt="device", adapt_metric=True, **kw)
    mean, var = H.sampling_stats(tg, Lc, out.draws[:, -1, :])
    plain = fn(result, A.SAMPLING_T, nwarmup=A.SAMPLING_W, rng=pfmi_mod.HostRNG(777), adapt="device", **kw)
    print("METRIC_SAMPLING gpu", sampler, np.max(np.abs(mean)), np.min(var), np.max(var), "accept", out.accept_prob.mean(), "eps", out.step_size.min(),
          out.step_size.max(), "without adapt_metric", plain.step_size.min(), plain.step_size.max(), "scale", out.metric_scale.min(),
          out.metric_scale.max())
    assert plain.metric_scale is None and sorted(plain.warmup) == ["accept_trace", "divergent", "eps_trace", "n_leapfrog", "status"]
    # (the engine's latest run is `plain`: run `out` again so that the CONTINUE below goes on from chains that carry the scale)
    out = fn(result, A.SAMPLING_T, nwarmup=A.SAMPLING_W, rng=pfmi_mod.HostRNG(777), adapt="device", adapt_metric=True, **kw)
    assert out.divergent.sum() == 0 and np.all(out.warmup["status"] == 0)
    assert H.sampling_ok(mean, var), (mean, var)
    assert out.metric_scale.shape == (H.SAMPLING_K, tg.d) and np.all(np.isfinite(out.metric_scale)) and np.all(out.metric_scale > 0)
    assert out.warmup["window_ends"].tolist() == [100] and np.array_equal(out.warmup["scale_trace"][:, -1], out.metric_scale)
    s = out.summary()
    assert s.nchains == H.SAMPLING_K and s.ndraws == A.SAMPLING_T and out.run == eng.hmc_runs and "chains: %d" % H.SAMPLING_K in str(out)
    # a CONTINUE afterwards uses the adapted scale: the metric kernel steps it
    plan = "%s_metric:%d:res" % (sampler, H.kpad_for(6))
    before = eng.kernel_time(plan)[1]
    sd = pfmi_mod.HostRNG(777).rand_u64(H.SAMPLING_K)
    if sampler == "hmc":
        eng.hmc_enqueue(out.metric_points, None, sd, out.step_size, H.SAMPLING_LF, 1, cont=True)
    else:
        eng.nuts_enqueue(out.metric_points, None, sd, out.step_size, 5, 1, cont=True)
    _wait(eng, sampler)
    assert eng.kernel_time(plan)[1] > before
    with pytest.raises(ValueError, match="device"):
        fn(result, 5, nwarmup=30, adapt="windows", adapt_metric=True, **kw)
