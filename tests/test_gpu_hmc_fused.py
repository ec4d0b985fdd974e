"""Fused static HMC on the built-in targets (include/pfmi.h: pfmi_hmc_fused_enqueue; pathfinder.jl_amd/csrc/hmc_fused_kernel.hip) beyond
the per-round checks of tests/test_gpu_hmc_fused_steps.py:

  * the fused loop equals its own single rounds bit for bit: the default launch cap, PFMI_HMC_FUSED_ROUNDS=1 (the rounds schedule) and
    =7 (which does not divide the 201 rounds and cuts trajectories), plain (K = 4, Lf = 5, T = 40) and adaptive (W = 25, T = 15, the traces
    of adapt_get included; the step-size trace within adapt_reference.bound of the long-double replay of its own acceptance trace);
  * PFMI_HMC_CONTINUE of 12 + 28 transitions is the run of 40, a chain run alone is its column at K = 4, and a CONTINUE after an adaptive
    run goes on from transition W + T;
  * divergent transitions leave the state alone; a start point with an infinite coordinate is PFMI_ERR_NUMERIC at the wait;
  * the sampling case of tests/hmc_reference.py (d = 8, 256 chains, T = 60, Lf = 4) on the built-in target;
  * the return codes through the C ABI, with the ctx usable after each, and the existing enqueues' refusal of a built-in target;
  * the public call pfmi.hmc on a built-in target in its three modes."""
import ctypes as C

import numpy as np
import pytest

import adapt_reference as A
import hmc_fused_reference as F
import hmc_reference as H
import margins as mg
from helpers import demo_device_target
from lbfgs_step_reference import HAVE_LONGDOUBLE

pytestmark = pytest.mark.gpu

ROWS = ("draws", "logp", "accept_prob", "energy_error", "divergent")


def _plain(eng, pts, x0, seeds, eps, T, cont=False, Lf=F.BIT_LF):
    eng.hmc_fused_enqueue(pts, None if cont else x0, seeds, eps, Lf, T, cont=cont)
    eng.hmc_wait()
    return eng.hmc_get()


def _adaptive(eng, pts, x0, seeds, eps0, W, T, Lf=F.BIT_LF):
    eng.hmc_fused_enqueue(pts, x0, seeds, eps0, Lf, T, nwarmup=W)
    eng.hmc_wait()
    return eng.hmc_get(), eng.adapt_get()


def _same(a, b, label):
    for q in a:
        assert np.array_equal(a[q], b[q]), (label, q)


@pytest.mark.parametrize("case", F.BIT_CASES, ids=[F.case_id(c) for c in F.BIT_CASES])
def test_the_fused_loop_equals_its_own_single_rounds_bit_for_bit(pfmi_mod, eng, case):
    d, J, tn = case
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=F.BIT_K)
    plan = F.plan_name(tg, d, H.kpad_for(J))
    rounds = 1 + F.BIT_T * F.BIT_LF
    runs, more, adapt = {}, {}, {}
    try:
        for cap in F.BIT_CAPS:
            F.set_round_cap(pfmi_mod, cap)
            n = -(-rounds // (cap or F.ROUNDS_CAP))
            before = eng.kernel_time(plan)[1]
            runs[cap] = _plain(eng, pts, x0, seeds, eps, F.BIT_T)
            assert eng.kernel_time(plan)[1] - before == n and eng.hmc_stats() == (rounds, 0), (cap, n)
            # the final state (x, lp, wg, the transition counter): two more transitions from it, under the same cut
            more[cap] = _plain(eng, pts, x0, seeds, eps, 2, cont=True)
            assert eng.hmc_stats() == (2 * F.BIT_LF, 0)
            adapt[cap] = _adaptive(eng, pts, x0, seeds, eps, F.BIT_W, F.BIT_TA)
            assert eng.hmc_stats() == (1 + (F.BIT_W + F.BIT_TA) * F.BIT_LF, 0)
    finally:
        F.set_round_cap(pfmi_mod, None)
    assert runs[None]["accept_prob"].min() < 1.0 and 0 < runs[None]["accept_prob"].mean()
    for cap in F.BIT_CAPS[1:]:
        _same(runs[None], runs[cap], ("plain", cap))
        _same(more[None], more[cap], ("continue", cap))
        _same(adapt[None][0], adapt[cap][0], ("adaptive rows", cap))
        _same(adapt[None][1], adapt[cap][1], ("adaptive traces", cap))
    got, warm = adapt[None]
    assert got["draws"].shape == (d, F.BIT_TA, F.BIT_K) and warm["eps_trace"].shape == (F.BIT_K, F.BIT_W)
    assert np.array_equal(warm["eps_trace"][:, 0], eps) and np.all(warm["status"] == 0) and np.all(warm["n_leapfrog"] == F.BIT_LF)
    if HAVE_LONGDOUBLE:
        worst = 0.0
        for k in range(F.BIT_K):
            acc, trace, final = warm["accept_trace"][k], warm["eps_trace"][k], float(warm["step_size"][k])
            be, bb, re, rb = A.bound(float(eps[k]), 0.8, acc)
            W = len(acc)
            q = [abs(float(A.LD(trace[m]) / re[m] - 1)) / be[m - 1] for m in range(1, W)] + [abs(float(A.LD(final) / rb[W - 1] - 1)) / bb[W - 1]]
            worst = max(worst, max(q))
        mg.check("hmc_fused:" + F.case_id(case), "hmc_fused_adapt_eps", [worst], 1.0)


def test_continue_and_independence_from_k(pfmi_mod, eng):
    case = F.BIT_CASES[0]
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=F.BIT_K)
    full = _plain(eng, pts, x0, seeds, eps, 40)
    a = _plain(eng, pts, x0, seeds, eps, 12)
    b = _plain(eng, pts, x0, seeds, eps, 28, cont=True)
    assert eng.hmc_stats() == (28 * F.BIT_LF, 0)
    for q in ROWS:
        assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), full[q]), q       # (draws (d, T, K), the others (K, T): T is axis 1)
    for k in range(F.BIT_K):
        one = _plain(eng, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps[k:k + 1], 40)
        assert np.array_equal(one["draws"][:, :, 0], full["draws"][:, :, k]), k
        for q in ROWS[1:]:
            assert np.array_equal(one[q][0], full[q][k]), (k, q)
    # after an adaptive run a CONTINUE goes on from transition W + T: rows 15 .. 19 of the adaptive run with 20 sampling transitions
    W, T = F.BIT_W, F.BIT_TA
    long_run, _ = _adaptive(eng, pts, x0, seeds, eps, W, T + 5)
    got, warm = _adaptive(eng, pts, x0, seeds, eps, W, T)
    tail = _plain(eng, pts, x0, seeds, warm["step_size"], 5, cont=True)
    for q in ROWS:
        assert np.array_equal(got[q], long_run[q][:, :T] if q != "draws" else long_run[q][:, :T, :]), q
        assert np.array_equal(tail[q], long_run[q][:, T:] if q != "draws" else long_run[q][:, T:, :]), q
    assert np.array_equal(eng.adapt_get()["step_size"], warm["step_size"])       # the adaptive run's, not the CONTINUE's copy


def _funnel10(pfmi_mod, eng):
    d = 10
    tg = pfmi_mod.t_funnel(d)
    eng.set_target(tg)
    eng.optimize_batch(pfmi_mod.HostRNG(5).rand(d).reshape(1, d) * 2 - 1, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert eng.fit_status()[0][0] == 0
    th, _, _ = eng.get_trace(0)
    return tg, np.asfortranarray(np.repeat(th[0][:, None], 2, axis=1))


def test_divergent_transitions_leave_the_state_alone_and_bad_starts_are_reported(pfmi_mod, eng):
    tg, x0 = _funnel10(pfmi_mod, eng)
    seeds = np.array([11, 12], dtype=np.uint64)
    got = _plain(eng, [0, 0], x0, seeds, np.array([1e200, 0.05]), 6, Lf=3)
    assert np.all(got["divergent"][0] == 1) and np.all(got["accept_prob"][0] == 0.0)
    assert np.array_equal(got["draws"][:, :, 0], np.repeat(x0[:, :1], 6, axis=1))                 # nothing non-finite entered the state
    assert np.all(got["logp"][0] == got["logp"][0, 0]) and np.isclose(got["logp"][0, 0], float(tg.logp(x0[:, 0])), rtol=1e-12, atol=0)
    assert np.all(np.isfinite(got["draws"])) and np.all(got["divergent"][1] == 0) and got["accept_prob"][1].mean() > 0.5
    xbad = x0.copy()
    xbad[3, 1] = np.inf
    eng.hmc_fused_enqueue([0, 0], xbad, seeds, 0.05, 3, 2)
    with pytest.raises(pfmi_mod.PfmiError) as ex:
        eng.hmc_wait()
    assert ex.value.code == -5 and "chain 1" in str(ex.value)                                     # PFMI_ERR_NUMERIC
    again = _plain(eng, [0, 0], x0, seeds, np.array([1e200, 0.05]), 6, Lf=3)                      # the ctx samples afterwards
    _same(got, again, "after a bad start")


def test_sampling_case_on_the_built_in_target(pfmi_mod, eng):
    tg, _, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(tg)
    eng.optimize_batch(pfmi_mod.HostRNG(3).rand(8).reshape(1, 8) * 4 - 2, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(8)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    got = _plain(eng, [0] * H.SAMPLING_K, X0, seeds, H.SAMPLING_EPS, H.SAMPLING_T, Lf=H.SAMPLING_LF)
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    print("HMC_FUSED_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), got["accept_prob"].mean())
    assert got["divergent"].sum() == 0
    assert H.sampling_ok(mean, var), (mean, var)


def test_return_codes_through_the_c_abi(pfmi_mod):
    d = 10
    tg = pfmi_mod.t_lowrank(d, r=2)
    L = pfmi_mod._lib.lib()
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.tile(tg.mean[:, None], (1, 2)))
    seeds = np.array([5, 6], dtype=np.uint64)
    dp, i64p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)

    def enq(k=2, pts=(0, 0), x=x0, sd=seeds, eps=(0.1, 0.1), lf=2, w=0, t=2, delta=0.8, flags=0):
        p = np.array(pts, dtype=np.int64)
        s = np.array(eps, dtype=np.float64)
        return L.pfmi_hmc_fused_enqueue(e.ctx, k, p.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp),
                                        None if sd is None else sd.ctypes.data_as(u64p), s.ctypes.data_as(dp), lf, w, t, C.c_double(delta), flags)

    try:
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        assert enq() == -3 and b"pfmi_fit_batch" in L.pfmi_last_error()                 # PFMI_ERR_STATE: not fitted
        e.fit_batch(6)
        for bad in (dict(k=0), dict(x=None), dict(sd=None), dict(lf=0), dict(t=0), dict(flags=4), dict(pts=(0, 10 ** 6)), dict(pts=(-1, 0)),
                    dict(eps=(0.1, 0.0)), dict(eps=(np.nan, 0.1)), dict(w=-1), dict(w=3, flags=1), dict(w=3, flags=2), dict(w=3, delta=0.0),
                    dict(w=3, delta=1.0)):
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG
            assert L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3            # ... which leaves no run behind
        assert enq(flags=1) == -3                                                       # PFMI_ERR_STATE: CONTINUE without chains
        assert enq() == 0 and L.pfmi_hmc_wait(e.ctx) == 0                               # the ctx is usable after the refusals
        r, n = C.c_int64(), C.c_int64()
        assert L.pfmi_hmc_stats(e.ctx, C.byref(r), C.byref(n)) == 0 and (r.value, n.value) == (5, 0)
        ptr, cnt = C.c_void_p(), C.c_int64()
        assert L.pfmi_hmc_draws_dev(e.ctx, C.byref(ptr), C.byref(cnt)) == 0 and ptr.value and cnt.value == 4
        assert L.pfmi_hmc_get_path(e.ctx, 0, 1, None, None, None) == -3                 # the run kept no path
        assert enq(flags=1) == 0 and enq(flags=1, k=1) == -3                            # CONTINUE with another K
        assert enq(flags=2) == 0 and L.pfmi_hmc_get_path(e.ctx, 0, 5, None, None, None) == 0
        assert enq(w=3) == 0 and L.pfmi_hmc_wait(e.ctx) == 0 and L.pfmi_adapt_get(e.ctx, None, None, None, None, None, None) == 0
        assert L.pfmi_hmc_stats(e.ctx, C.byref(r), C.byref(n)) == 0 and (r.value, n.value) == (1 + 5 * 2, 0)
        # a staged scale: the metric kernels are not fused
        scale = np.ones((2, d))
        assert L.pfmi_chain_scale_set(e.ctx, 2, scale.ctypes.data_as(dp)) == 0
        assert enq() == -4 and b"scale" in L.pfmi_last_error()
        assert L.pfmi_chain_scale_set(e.ctx, 0, None) == 0
        assert enq() == 0 and L.pfmi_hmc_wait(e.ctx) == 0
        # after the new runs, the existing enqueues still refuse the built-in target
        p = np.zeros(2, dtype=np.int64)
        s = np.full(2, 0.1)
        head = (e.ctx, 2, p.ctypes.data_as(i64p), x0.ctypes.data_as(dp), seeds.ctypes.data_as(u64p), s.ctypes.data_as(dp))
        assert L.pfmi_hmc_enqueue(*head, 2, 2, 0) == -4
        assert L.pfmi_nuts_enqueue(*head, 3, 2, 0) == -4
        assert L.pfmi_hmc_adapt_enqueue(*head, 2, 3, 2, C.c_double(0.8), 0) == -4
        assert L.pfmi_nuts_adapt_enqueue(*head, 3, 3, 2, C.c_double(0.8), 0) == -4
        assert L.pfmi_chees_enqueue(e.ctx, 2, p.ctypes.data_as(i64p), x0.ctypes.data_as(dp), seeds.ctypes.data_as(u64p), C.c_double(0.1),
                                    C.c_double(0.0), 8, 3, 2, C.c_double(0.651), 0) == -4
        assert enq() == 0 and L.pfmi_hmc_wait(e.ctx) == 0
        # any callback target: PFMI_ERR_UNSUPPORTED, with the entry point that serves it in the message
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq() == -4 and b"pfmi_hmc_enqueue" in L.pfmi_last_error()
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq() == 0 and L.pfmi_hmc_wait(e.ctx) == 0
    finally:
        e.close()


def test_public_hmc_call_on_a_built_in_target(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(pfmi_mod.t_lowrank(20, r=2), 8, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        res = pfmi_mod.resample(res, 6, replace=False, rng=pfmi_mod.HostRNG(5))
        fixed = pfmi_mod.hmc(res, 12, step_size=0.2, nleapfrog=4)
        assert isinstance(fixed, pfmi_mod.HMCResult) and fixed.draws.shape == (20, 12, 6) and np.all(fixed.step_size == 0.2)
        assert e.hmc_stats() == (1 + 12 * 4, 0)
        win = pfmi_mod.hmc(res, 20, nwarmup=20, rng=pfmi_mod.HostRNG(8))
        dev = pfmi_mod.hmc(res, 20, nwarmup=20, adapt="device", rng=pfmi_mod.HostRNG(8))
        for out in (win, dev):
            assert out.draws.shape == (20, 20, 6) and np.all(np.isfinite(out.draws)) and out.nwarmup == 20 and out.nleapfrog == 8
            for q in (out.logp, out.accept_prob, out.energy_error, out.divergent):
                assert q.shape == (6, 20)
            assert out.step_size.shape == (6,) and np.all(out.step_size > 0) and np.all(out.step_size != 20 ** -0.25)
            assert "chains: 6" in str(out) and "Static HMC" in str(out) and "(warm-up: 20)" in str(out)
        assert win.warmup is None and dev.warmup["eps_trace"].shape == (6, 20) and dev.metric_scale is None
        s = dev.summary()                                              # served from the resident records
        assert s.nchains == 6 and s.ndraws == 20 and s.rhat.shape == (20,) and np.all(np.isfinite(s.mean)) and np.isfinite(s.lp["ess_bulk"])
        host = pfmi_mod.chain_diagnostics(dev.draws, e)
        assert np.array_equal(s.mean, host["mean"]) and np.array_equal(s.ess_bulk, host["ess_bulk"])
        with pytest.raises(ValueError, match="static HMC is available"):
            pfmi_mod.hmc(res, 5, nwarmup=30, adapt="device", adapt_metric=True)
        with pytest.raises(ValueError, match="static HMC is available"):
            pfmi_mod.nuts(res, 5)
        with pytest.raises(ValueError, match="static HMC is available"):
            pfmi_mod.chees(res, 5)
    finally:
        e.close()
