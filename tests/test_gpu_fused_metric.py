"""The metric windows and scaled chains on the built-in targets (include/pfmi.h: pfmi_hmc_fused_metric_enqueue,
pfmi_nuts_fused_metric_enqueue; csrc/hmc_fused_metric_kernel.hip, csrc/nuts_fused_metric_kernel.hip), both samplers, with the parameters
of tests/metric_adapt_reference.py (Lf = 3, max_depth 4, K = 3, delta = 0.8) on the chains of hmc_fused_reference.setup_chains:

  1. an adaptive run is BIT-IDENTICAL to a host-driven replay of its own step-size and scale traces through the same entry point with
     nwarmup = 0 and pfmi_chain_scale_set, and its whitened rows, window scales and step-size segments are within the bounds of
     metric_adapt_reference.check_run (counted from the operations there) of the long-double references;
  2. the loop equals its own single trips: the launch caps None, 1 and 7 give the same bits (cap 1 puts a launch boundary back between a
     window's end, which writes the scale, and the kick that reads it), NUTS also pumped against waited;
  3. a staged scale of ones gives the bits of pfmi_*_fused_enqueue, on the *_fused_metric plan;
  4. a plain RECORD_PATH run on a random scale passes the step checkers on ScaledMetric and the long-double target;
  5. CONTINUE and independence from K with a scale;
  6. a warm-up below 20 transitions is the fused step-size warm-up;
  7. the return codes through the C ABI;
  8. the sampling case, through the public calls with adapt_metric="fused";
  9. the public calls.
Largest ratios seen: profiles/fused_metric_parity.md."""
import ctypes as C
import types

import numpy as np
import pytest

import adapt_reference as A
import hmc_fused_reference as F
import hmc_reference as H
import metric_adapt_reference as MA
import nuts_fused_reference as NF
import nuts_reference as N
from helpers import demo_device_target
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

pytestmark = pytest.mark.gpu

K = H.GRID_K
SAMPLERS = ("hmc", "nuts")
PARAM = {"hmc": MA.LF, "nuts": MA.DEPTH}
# (d, J, target, W, T): two windows [75, 100), [100, 150) -- the doubling and both restarts -- where a transition is cheap; one window
# [3, 18) where one thread owns two rows (rank padding 16 and 0) and on the streamed side of pf_hmc_resident at KPAD 12
CASES = [(5, 2, "gauss", 200, 4), (5, 2, "funnel", 200, 4), (64, 6, "gauss", 200, 4), (64, 6, "funnel", 200, 4),
         (257, 6, "lowrank12", 20, 2), (257, 16, "diag", 20, 2), (1601, 6, "funnel", 20, 2)]


def _cid(case):
    return F.case_id(case[:3])


def _plan(sampler, tg, d, J, metric=True):
    kpad = H.kpad_for(J)
    return "%s_fused%s:%d:%s:%s" % (sampler, "_metric" if metric else "", kpad, "res" if H.resident(d, kpad) else "stream", F.target_tag(tg))


def _count(eng, plan):
    return eng.kernel_time(plan)[1]


def _wait(eng, sampler, pump=False):
    if sampler == "hmc":
        eng.hmc_wait()
        return
    if pump:
        passes = 0
        while not eng.nuts_pump():
            passes += 1
            assert passes < 10 ** 8
    eng.nuts_wait()


def _rows(eng, sampler):
    got = eng.hmc_get()
    if sampler == "nuts":
        got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got


def _run(eng, sampler, pts, x0, seeds, eps, T, W=0, cont=False, record_path=False, record_whitened=False, pump=False, metric=True):
    """one call of the new entry point (metric=False: of pfmi_*_fused_enqueue) and its rows"""
    kw = dict(nwarmup=W, cont=cont, record_path=record_path)
    if metric:
        fn = eng.hmc_fused_metric_enqueue if sampler == "hmc" else eng.nuts_fused_metric_enqueue
        kw["record_whitened"] = record_whitened
    else:
        fn = eng.hmc_fused_enqueue if sampler == "hmc" else eng.nuts_fused_enqueue
    fn(pts, None if cont else x0, seeds, eps, PARAM[sampler], T, **kw)
    _wait(eng, sampler, pump)
    return _rows(eng, sampler)


def _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T, pump=False):
    got = _run(eng, sampler, pts, x0, seeds, eps0, T, W=W, record_whitened=True, pump=pump)
    return got, eng.adapt_get(), eng.adapt_metric_get()


def _same(a, b, label):
    assert sorted(a) == sorted(b), label
    for q in a:
        assert np.array_equal(a[q], b[q]), (label, q)


def _replay(eng, sampler, pts, x0, seeds, got, warm, met, W, T, label):
    """the run's own traces through the new entry point with nwarmup = 0: one transition per call with the recorded step size, the
    recorded scale of window j staged in front of transition ends[j]; then one call of T.  Returns the states after the warm-up
    transitions (K, W, d)."""
    ends = met["window_ends"].tolist()
    states = np.empty((len(pts), W, x0.shape[0]))
    for t in range(W):
        if t in ends:
            eng.chain_scale_set(met["scale_trace"][:, ends.index(t)])
        one = _run(eng, sampler, pts, x0, seeds, warm["eps_trace"][:, t], 1, cont=t > 0)
        assert np.array_equal(one["accept_prob"][:, 0], warm["accept_trace"][:, t]), (label, t, one["accept_prob"][:, 0], warm["accept_trace"][:, t])
        assert np.array_equal(one["divergent"][:, 0], warm["divergent"][:, t]), (label, t)
        if sampler == "nuts":
            assert np.array_equal(one["n_leapfrog"][:, 0], warm["n_leapfrog"][:, t]), (label, t)
        else:
            assert np.all(warm["n_leapfrog"][:, t] == MA.LF)
        states[:, t] = one["draws"][:, 0, :].T
    last = _run(eng, sampler, pts, x0, seeds, warm["step_size"], T, cont=True)
    _same(last, got, label)
    return states


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_adaptive_run_is_bit_identical_to_its_replay_and_matches_the_references(pfmi_mod, eng, case, sampler):
    d, J, tn, W, T = case
    kpad = H.kpad_for(J)
    label = (_cid(case), sampler)
    tg, pts, x0, eps0, seeds, jeff = F.setup_chains(pfmi_mod, eng, case[:3], K=K)
    init, _, ends = MA.windows(W)
    plan, other = _plan(sampler, tg, d, J), _plan(sampler, tg, d, J, metric=False)
    before, obefore = _count(eng, plan), _count(eng, other)
    got, warm, met = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T)
    launches = _count(eng, plan) - before
    assert _count(eng, other) == obefore                        # every launch of the run was a fused-metric one
    if sampler == "hmc":
        rounds = 1 + (W + T) * MA.LF
        assert launches == -(-rounds // F.ROUNDS_CAP) and eng.hmc_stats() == (rounds, 0), (label, launches)
    else:
        trips = 1 + int(np.max(np.sum(warm["n_leapfrog"], axis=1) + np.sum(got["n_leapfrog"], axis=1)))
        assert eng.nuts_stats() == (trips, 0) and launches >= -(-trips // NF.ROUNDS_CAP), (label, launches, trips)
    assert met["window_ends"].tolist() == ends and met["scale_trace"].shape == (K, len(ends), d)
    assert met["whitened"].shape == (K, ends[-1] - init, d) and got["draws"].shape == (d, T, K)
    assert np.all(np.isfinite(met["scale_trace"])) and np.all(met["scale_trace"] > 0)
    assert np.all(warm["status"] == 0), (label, warm["status"])                   # (no KEPT_METRIC: the checker below checks every window's scale)
    assert np.array_equal(warm["eps_trace"][:, 0], eps0) and np.all(np.isfinite(warm["eps_trace"])) and np.all(warm["eps_trace"] > 0)
    states = _replay(eng, sampler, pts, x0, seeds, got, warm, met, W, T, label)
    if HAVE_LONGDOUBLE:
        margins = {}
        for k in range(K):
            M = H.Metric.from_fit(eng.get_fit(int(pts[k]), int(jeff[int(pts[k])])))
            run = {"states": states[k], "whitened": met["whitened"][k], "scale_trace": met["scale_trace"][k], "eps_trace": warm["eps_trace"][k],
                   "accept_trace": warm["accept_trace"][k], "step_size": warm["step_size"][k]}
            for q, v in MA.check_run(M, kpad, x0[:, k], W, 0.8, run).items():
                margins[q] = max(margins.get(q, 0.0), v)
        print("FUSED_METRIC_PARITY gpu", sampler, _cid(case), "largest error / bound", {q: float("%.3g" % v) for q, v in margins.items()})
        assert sorted(margins) == ["eps", "scale", "whiten"] and max(margins.values()) <= 1.0, margins


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("case", [(64, 6, "gauss"), (257, 6, "funnel")], ids=F.case_id)
def test_the_loop_equals_its_own_single_trips_bit_for_bit(pfmi_mod, eng, case, sampler):
    """a launch cap of 1 puts the launch boundary of the step kernels back between the end of a window (the scale is written) and the
    next kick (it is read): the default cap, where both happen in one launch, must give the same bits"""
    W, T = F.BIT_W, F.BIT_TA
    assert MA.windows(W) == (3, 2, [23])                        # one window [3, 23): warm-up transitions 23 and 24 and the sampling use its scale
    tg, pts, x0, eps0, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=K)
    set_cap = F.set_round_cap if sampler == "hmc" else NF.set_round_cap
    plan = _plan(sampler, tg, case[0], case[1])
    runs, launches = {}, {}
    try:
        for cap in (None, 1, 7):
            set_cap(pfmi_mod, cap)
            before = _count(eng, plan)
            runs[cap] = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T)
            launches[cap] = _count(eng, plan) - before
        if sampler == "nuts":
            set_cap(pfmi_mod, 7)
            runs["pumped"] = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T, pump=True)
    finally:
        set_cap(pfmi_mod, None)
    got, warm, met = runs[None]
    assert launches[None] == 1 and launches[1] > launches[7] > 1, launches
    assert np.all(warm["status"] == 0) and not np.array_equal(met["scale_trace"], np.ones_like(met["scale_trace"]))
    if sampler == "hmc":
        assert launches[1] == 1 + (W + T) * MA.LF and launches[7] == -(-launches[1] // 7), launches
    for cap in list(runs)[1:]:
        for a, b, what in zip(runs[None], runs[cap], ("rows", "traces", "windows")):
            _same(a, b, (sampler, what, cap))


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_a_scale_of_ones_gives_the_bits_of_the_fused_enqueue(pfmi_mod, eng, sampler):
    case = (64, 6, "funnel")
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=K)
    plain = _run(eng, sampler, pts, x0, seeds, eps, F.GRID_T, metric=False)
    plan, other = _plan(sampler, tg, 64, 6), _plan(sampler, tg, 64, 6, metric=False)
    before, obefore = _count(eng, plan), _count(eng, other)
    eng.chain_scale_set(np.ones((K, 64)))
    ones = _run(eng, sampler, pts, x0, seeds, eps, F.GRID_T)
    assert _count(eng, plan) - before == 1 and _count(eng, other) == obefore
    _same(plain, ones, sampler)
    # without a scale the new entry point runs the fused kernel itself
    none = _run(eng, sampler, pts, x0, seeds, eps, F.GRID_T)
    assert _count(eng, plan) - before == 1 and _count(eng, other) - obefore == 1
    _same(plain, none, sampler)


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)
@pytest.mark.parametrize("case", [(5, 10, "gauss"), (64, 6, "funnel"), (257, 6, "lowrank12")], ids=F.case_id)
def test_plain_run_on_a_random_scale_passes_the_step_checkers(pfmi_mod, eng, case):
    d, J, tn = case
    T, kpad = H.GRID_T, H.kpad_for(J)
    tg, pts, x0, eps, seeds, jeff = F.setup_chains(pfmi_mod, eng, case, K=K)
    scale = 0.5 + 1.5 * np.random.default_rng(d + J).random((K, d))
    for sampler in SAMPLERS:
        plan = _plan(sampler, tg, d, J)
        before = _count(eng, plan)
        eng.chain_scale_set(scale)
        got = _run(eng, sampler, pts, x0, seeds, eps, T, record_path=True)
        assert _count(eng, plan) - before == 1
        path = eng.hmc_path() if sampler == "hmc" else eng.nuts_path()
        stats = (got["tree_depth"], got["n_leapfrog"]) if sampler == "nuts" else None
        borderline = decisions = 0
        for k in range(K):
            p = int(pts[k])
            S = MA.ScaledMetric(H.Metric.from_fit(eng.get_fit(p, int(jeff[p]))), scale[k])
            if sampler == "hmc":
                rec = H.gpu_recording(x0[:, k], path, got, k)
                o = H.check(S, rec, int(seeds[k]), float(eps[k]), MA.LF, kpad, label=(case, k))
                decisions += T
            else:
                rec = N.gpu_recording(x0[:, k], path, got, stats, k)
                o = N.check(S, rec, int(seeds[k]), float(eps[k]), MA.DEPTH, kpad, label=(case, k))
                decisions += o["decisions"]
            borderline += o["borderline"]
            rl, rg = F.target_ratios(tg, rec["X"], rec["lp"], rec["g"])
            print("FUSED_METRIC_STEP", sampler, F.case_id(case), k, {q: float("%.3g" % m) for q, m in o["margins"].items()}, "lp", float("%.3g" % rl),
                  "grad", float("%.3g" % rg))
            assert max(o["margins"].values()) <= 1.0 and rl <= 1.0 and rg <= 1.0, (sampler, k, o["margins"], rl, rg)
        assert borderline <= (2 * decisions) // 100, (sampler, borderline, decisions)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_continue_and_independence_from_k_with_a_scale(pfmi_mod, eng, sampler):
    case = (64, 6, "gauss")
    T = 6
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=K)
    scale = 0.5 + 1.5 * np.random.default_rng(7).random((K, 64))
    plan = _plan(sampler, tg, 64, 6)
    eng.chain_scale_set(scale)
    full = _run(eng, sampler, pts, x0, seeds, eps, 2 * T)
    unscaled = _run(eng, sampler, pts, x0, seeds, eps, 2 * T)
    assert not np.array_equal(unscaled["draws"], full["draws"])                    # the scale was used, and a fresh run forgets it
    eng.chain_scale_set(scale)
    a = _run(eng, sampler, pts, x0, seeds, eps, T)
    before = _count(eng, plan)
    b = _run(eng, sampler, pts, x0, seeds, eps, T, cont=True)                      # the chains carry their scale
    assert _count(eng, plan) - before == 1
    for q in full:
        assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), full[q]), q   # (draws (d, T, K), the others (K, T): T is axis 1)
    for k in range(K):
        eng.chain_scale_set(scale[k:k + 1])
        one = _run(eng, sampler, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps[k:k + 1], 2 * T)
        assert np.array_equal(one["draws"][:, :, 0], full["draws"][:, :, k]), k
        for q in full:
            if q != "draws":
                assert np.array_equal(one[q][0], full[q][k]), (k, q)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_short_warm_up_is_the_fused_step_size_warm_up(pfmi_mod, eng, sampler):
    case = (64, 6, "gauss")
    tg, pts, x0, eps0, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=K)
    plan, other = _plan(sampler, tg, 64, 6), _plan(sampler, tg, 64, 6, metric=False)
    a_got = _run(eng, sampler, pts, x0, seeds, eps0, 3, W=12, metric=False)
    a_warm = eng.adapt_get()
    before, obefore = _count(eng, plan), _count(eng, other)
    m_got = _run(eng, sampler, pts, x0, seeds, eps0, 3, W=12)
    m_warm, met = eng.adapt_get(), eng.adapt_metric_get()
    assert _count(eng, plan) == before and _count(eng, other) > obefore            # only the fused plan's counter moved
    _same(a_got, m_got, sampler)
    for q in a_warm:
        if q != "status":
            assert np.array_equal(a_warm[q], m_warm[q]), q
    assert np.all(a_warm["status"] == 0) and np.all(m_warm["status"] == MA.NO_METRIC_WINDOW)
    assert len(met["window_ends"]) == 0 and met["scale_trace"].shape == (K, 0, 64)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_return_codes_through_the_c_abi(pfmi_mod, sampler):
    d = 20
    tg = pfmi_mod.t_lowrank(d, r=2)
    L = pfmi_mod._lib.lib()
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.tile(tg.mean[:, None], (1, 2)))
    seeds = np.array([5, 6], dtype=np.uint64)
    dp, i64p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    new, old, wait = ((L.pfmi_hmc_fused_metric_enqueue, L.pfmi_hmc_fused_enqueue, L.pfmi_hmc_wait) if sampler == "hmc" else
                      (L.pfmi_nuts_fused_metric_enqueue, L.pfmi_nuts_fused_enqueue, L.pfmi_nuts_wait))

    def enq(fn=new, k=2, pts=(0, 0), x=x0, sd=seeds, eps=(0.1, 0.1), par=2, w=0, t=2, delta=0.8, flags=0):
        p = np.array(pts, dtype=np.int64)
        s = np.array(eps, dtype=np.float64)
        return fn(e.ctx, k, p.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp), None if sd is None else sd.ctypes.data_as(u64p),
                  s.ctypes.data_as(dp), par, w, t, C.c_double(delta), flags)

    def no_run():
        return L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3

    def metric_get():
        return L.pfmi_adapt_metric_get(e.ctx, None, None, None, None)

    try:
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        assert enq() == -3 and b"pfmi_fit_batch" in L.pfmi_last_error()                 # PFMI_ERR_STATE: not fitted
        e.fit_batch(6)
        bad_param = [dict(par=0)] if sampler == "hmc" else [dict(par=0), dict(par=11)]
        for bad in [dict(k=0), dict(x=None), dict(sd=None), dict(t=0), dict(flags=4), dict(flags=8), dict(pts=(0, 10 ** 6)), dict(pts=(-1, 0)),
                    dict(eps=(0.1, 0.0)), dict(eps=(np.nan, 0.1)), dict(w=-1), dict(w=25, flags=1), dict(w=25, flags=2), dict(w=25, flags=5),
                    dict(w=25, flags=8), dict(w=25, delta=0.0), dict(w=25, delta=1.0)] + bad_param:
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG ...
            assert no_run(), bad                                                        # ... which leaves no run behind
        assert enq(flags=1) == -3                                                       # PFMI_ERR_STATE: CONTINUE without chains
        assert enq() == 0 and wait(e.ctx) == 0 and metric_get() == -3                   # a run without windows serves no pfmi_adapt_metric_get
        assert enq(flags=1) == 0 and enq(flags=1, k=1) == -3 and no_run()               # CONTINUE with another K
        assert enq(w=25) == 0 and wait(e.ctx) == 0 and metric_get() == 0
        assert enq(w=25, flags=MA.RECORD_WHITENED) == 0 and wait(e.ctx) == 0 and metric_get() == 0
        # the chains of that run carry a scale: the new entry point goes on with them, the fused enqueue keeps refusing them
        assert enq(flags=1) == 0 and wait(e.ctx) == 0
        assert enq(fn=old, flags=1) == -4 and b"scale" in L.pfmi_last_error() and no_run()
        scale = np.full((2, d), 1.5)
        assert L.pfmi_chain_scale_set(e.ctx, 2, scale.ctypes.data_as(dp)) == 0
        assert enq(fn=old) == -4 and b"scale" in L.pfmi_last_error()                    # (the refused call took the staging with it)
        assert L.pfmi_chain_scale_set(e.ctx, 2, scale.ctypes.data_as(dp)) == 0
        assert enq() == 0 and wait(e.ctx) == 0 and metric_get() == -3
        assert enq(fn=old, flags=1) == -4 and no_run()
        # a scale staged for another K
        assert L.pfmi_chain_scale_set(e.ctx, 3, np.ones((3, d)).ctypes.data_as(dp)) == 0
        assert enq() == -1 and no_run()
        assert enq() == 0 and wait(e.ctx) == 0
        # a callback target: PFMI_ERR_UNSUPPORTED, with the entry point that serves it in the message
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq(w=25) == -4 and b"adapt_metric_enqueue" in L.pfmi_last_error()
        assert enq() == -4 and b"adapt_metric_enqueue" in L.pfmi_last_error()
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq(w=25) == 0 and wait(e.ctx) == 0 and metric_get() == 0                # the ctx is usable after the refusals
    finally:
        e.close()


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_chains_sample_the_target_after_the_fused_metric_warm_up(pfmi_mod, eng, sampler):
    """the sampling case of test_gpu_hmc_fused.test_sampling_case_on_the_built_in_target, through pfmi.hmc / pfmi.nuts with
    adapt_metric="fused" and the warm-up of the closure route's metric sampling test"""
    tg, _, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(tg)
    eng.optimize_batch(pfmi_mod.HostRNG(3).rand(8).reshape(1, 8) * 4 - 2, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(8)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    result = types.SimpleNamespace(draws=X0, fit_distribution=types.SimpleNamespace(engine=eng, point=0, token=eng.fit_token()))
    fn, kw = (pfmi_mod.hmc, dict(nleapfrog=H.SAMPLING_LF)) if sampler == "hmc" else (pfmi_mod.nuts, dict(max_depth=5))
    plan = _plan(sampler, tg, 8, 6)
    before = _count(eng, plan)
    out = fn(result, A.SAMPLING_T, nwarmup=A.SAMPLING_W, rng=pfmi_mod.HostRNG(777), adapt="device", adapt_metric="fused", **kw)
    assert _count(eng, plan) > before
    mean, var = H.sampling_stats(tg, Lc, out.draws[:, -1, :])
    print("FUSED_METRIC_SAMPLING gpu", sampler, np.max(np.abs(mean)), np.min(var), np.max(var), "accept", out.accept_prob.mean(), "eps",
          out.step_size.min(), out.step_size.max(), "scale", out.metric_scale.min(), out.metric_scale.max())
    assert out.divergent.sum() == 0 and np.all(out.warmup["status"] == 0)
    assert H.sampling_ok(mean, var), (mean, var)
    assert out.metric_scale.shape == (H.SAMPLING_K, tg.d) and np.all(np.isfinite(out.metric_scale)) and np.all(out.metric_scale > 0)
    assert np.array_equal(out.warmup["scale_trace"][:, -1], out.metric_scale)
    assert out.warmup["window_ends"].tolist() == MA.windows(A.SAMPLING_W)[2]


def test_public_calls_on_a_built_in_target(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(pfmi_mod.t_lowrank(20, r=2), 8, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        res = pfmi_mod.resample(res, 6, replace=False, rng=pfmi_mod.HostRNG(5))
        calls = ((pfmi_mod.hmc, dict(), pfmi_mod.HMCResult), (pfmi_mod.nuts, dict(max_depth=5), pfmi_mod.NUTSResult),
                 (pfmi_mod.nuts, dict(max_depth=5, fused=True), pfmi_mod.NUTSResult))
        for fn, kw, cls in calls:
            out = fn(res, 20, nwarmup=30, adapt="device", adapt_metric="fused", rng=pfmi_mod.HostRNG(8), **kw)
            assert isinstance(out, cls) and out.draws.shape == (20, 20, 6) and np.all(np.isfinite(out.draws)) and out.nwarmup == 30
            assert out.metric_scale.shape == (6, 20) and np.all(np.isfinite(out.metric_scale)) and np.all(out.metric_scale > 0)
            assert out.warmup["window_ends"].tolist() == [27] and out.warmup["scale_trace"].shape == (6, 1, 20)
            assert np.array_equal(out.warmup["scale_trace"][:, 0], out.metric_scale) and out.warmup["eps_trace"].shape == (6, 30)
            s = out.summary()                                          # served from the resident records
            assert out.run == e.hmc_runs and s.nchains == 6 and s.ndraws == 20 and s.rhat.shape == (20,) and np.all(np.isfinite(s.mean))
            host = pfmi_mod.chain_diagnostics(out.draws, e)
            assert np.array_equal(s.mean, host["mean"]) and np.array_equal(s.ess_bulk, host["ess_bulk"])
        for fn in (pfmi_mod.hmc, pfmi_mod.nuts):
            with pytest.raises(ValueError, match="device"):
                fn(res, 5, nwarmup=30, adapt="windows", adapt_metric="fused")
            with pytest.raises(ValueError, match="adapt_metric"):
                fn(res, 5, nwarmup=30, adapt="device", adapt_metric="windows")
            with pytest.raises(ValueError, match="static HMC is available|adapt_metric"):
                fn(res, 5, nwarmup=30, adapt="device", adapt_metric=True, **(dict(fused=True) if fn is pfmi_mod.nuts else {}))
        # a closure target has the closure route: adapt_metric=True
        import torch
        tgt = pfmi_mod.t_diag(10, 1)
        m, a = torch.tensor(tgt.mean, device="cuda"), torch.tensor(tgt.a, device="cuda")
        clo = pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tgt, grad="autograd")
        res2 = pfmi_mod.multipathfinder(clo, 6, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        for fn in (pfmi_mod.hmc, pfmi_mod.nuts):
            with pytest.raises(ValueError, match="built-in target"):
                fn(res2, 5, nwarmup=30, adapt="device", adapt_metric="fused")
    finally:
        e.close()
