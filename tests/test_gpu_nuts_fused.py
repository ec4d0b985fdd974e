"""Fused NUTS on the built-in targets (include/pfmi.h: pfmi_nuts_fused_enqueue; pathfinder.jl_amd/csrc/nuts_fused_kernel.hip) beyond the
per-trip checks of tests/test_gpu_nuts_fused_steps.py:

  * the fused loop equals its own single trips bit for bit: the default launch cap, PFMI_NUTS_FUSED_ROUNDS=1 (the rounds schedule of the
    closure route) and =7 (which cuts trees), plain (K = 4, max_depth 5, T = 20, the chains' final states through two more transitions) and
    adaptive (W = 12, T = 8, the traces of adapt_get included); at cap 7 the launches are within the pump's window of ceil(trips / 7);
  * PFMI_NUTS_CONTINUE of T + T transitions is the run of 2 T, a chain run alone is its column at K = 4, and pumping with nuts_pump at
    cap 7 is the run of nuts_wait;
  * divergent transitions leave the state alone and are flagged; a start point with an infinite coordinate is PFMI_ERR_NUMERIC at the wait;
  * the sampling case of tests/test_gpu_hmc_fused.py (d = 8, 256 chains) with NUTS, judged by hmc_reference.sampling_ok;
  * the return codes through the C ABI in their order, with no run left behind and the ctx usable after each, and the existing enqueues'
    refusal of a built-in target;
  * the public call pfmi.nuts(..., fused=True) on a built-in target in its three modes, and the default's unchanged refusal."""
import ctypes as C

import numpy as np
import pytest

import hmc_fused_reference as F
import hmc_reference as H
import nuts_fused_reference as NF
from helpers import demo_device_target

pytestmark = pytest.mark.gpu

ROWS = ("draws", "logp", "accept_prob", "energy_error", "divergent", "tree_depth", "n_leapfrog")


def _get(eng):
    got = eng.hmc_get()
    got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got


def _plain(eng, pts, x0, seeds, eps, T, cont=False, md=NF.BIT_DEPTH, pump=False):
    eng.nuts_fused_enqueue(pts, None if cont else x0, seeds, eps, md, T, cont=cont)
    if pump:
        passes = 0
        while not eng.nuts_pump():
            passes += 1
            assert passes < 10 ** 8
    eng.nuts_wait()
    return _get(eng)


def _adaptive(eng, pts, x0, seeds, eps0, W, T, md=NF.BIT_DEPTH):
    eng.nuts_fused_enqueue(pts, x0, seeds, eps0, md, T, nwarmup=W)
    eng.nuts_wait()
    return _get(eng), eng.adapt_get()


def _same(a, b, label):
    for q in a:
        assert np.array_equal(a[q], b[q]), (label, q)


@pytest.mark.parametrize("case", NF.BIT_CASES, ids=[NF.case_id(c) for c in NF.BIT_CASES])
def test_the_fused_loop_equals_its_own_single_trips_bit_for_bit(pfmi_mod, eng, case):
    d, J, tn = case
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=NF.BIT_K)
    plan = NF.plan_name(tg, d, H.kpad_for(J))
    runs, more, adapt = {}, {}, {}
    try:
        for cap in NF.BIT_CAPS:
            NF.set_round_cap(pfmi_mod, cap)
            before = eng.kernel_time(plan)[1]
            runs[cap] = _plain(eng, pts, x0, seeds, eps, NF.BIT_T)
            launches = eng.kernel_time(plan)[1] - before
            trips = 1 + int(np.max(np.sum(runs[cap]["n_leapfrog"], axis=1)))
            assert eng.nuts_stats() == (trips, 0), (cap, eng.nuts_stats(), trips)
            lo, hi = NF.launches_bound(trips, cap or NF.ROUNDS_CAP)
            assert (launches == 1) if cap is None else (lo <= launches <= hi), (cap, launches, trips)
            # the final state (x, lp, wg, the transition counter): two more transitions from it, under the same cut
            more[cap] = _plain(eng, pts, x0, seeds, eps, 2, cont=True)
            assert eng.nuts_stats() == (int(np.max(np.sum(more[cap]["n_leapfrog"], axis=1))), 0)
            adapt[cap] = _adaptive(eng, pts, x0, seeds, eps, NF.BIT_W, NF.BIT_TA)
            warm_leaves = np.sum(adapt[cap][1]["n_leapfrog"], axis=1) + np.sum(adapt[cap][0]["n_leapfrog"], axis=1)
            assert eng.nuts_stats() == (1 + int(np.max(warm_leaves)), 0)
    finally:
        NF.set_round_cap(pfmi_mod, None)
    base = runs[None]
    assert base["accept_prob"].min() < 1.0 and 0 < base["accept_prob"].mean() and len(set(np.sum(base["n_leapfrog"], axis=1).tolist())) > 1
    for cap in NF.BIT_CAPS[1:]:
        _same(base, runs[cap], ("plain", cap))
        _same(more[None], more[cap], ("continue", cap))
        _same(adapt[None][0], adapt[cap][0], ("adaptive rows", cap))
        _same(adapt[None][1], adapt[cap][1], ("adaptive traces", cap))
    got, warm = adapt[None]
    assert got["draws"].shape == (d, NF.BIT_TA, NF.BIT_K) and warm["eps_trace"].shape == (NF.BIT_K, NF.BIT_W)
    assert np.array_equal(warm["eps_trace"][:, 0], eps) and np.all(warm["status"] == 0) and np.all(warm["n_leapfrog"] >= 1)
    assert np.all(warm["step_size"] > 0) and not np.array_equal(warm["step_size"], eps)


def test_continue_pump_and_independence_from_k(pfmi_mod, eng):
    case = NF.BIT_CASES[0]
    T = NF.BIT_T // 2
    tg, pts, x0, eps, seeds, _ = F.setup_chains(pfmi_mod, eng, case, K=NF.BIT_K)
    full = _plain(eng, pts, x0, seeds, eps, 2 * T)
    a = _plain(eng, pts, x0, seeds, eps, T)
    b = _plain(eng, pts, x0, seeds, eps, T, cont=True)
    assert eng.nuts_stats() == (int(np.max(np.sum(b["n_leapfrog"], axis=1))), 0)
    for q in ROWS:
        assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), full[q]), q       # (draws (d, T, K), the others (K, T): T is axis 1)
    for k in range(NF.BIT_K):
        one = _plain(eng, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps[k:k + 1], 2 * T)
        assert np.array_equal(one["draws"][:, :, 0], full["draws"][:, :, k]), k
        for q in ROWS[1:]:
            assert np.array_equal(one[q][0], full[q][k]), (k, q)
    try:
        NF.set_round_cap(pfmi_mod, 7)
        pumped = _plain(eng, pts, x0, seeds, eps, 2 * T, pump=True)
    finally:
        NF.set_round_cap(pfmi_mod, None)
    _same(full, pumped, "pumped at cap 7")


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
    got = _plain(eng, [0, 0], x0, seeds, np.array([1e200, 0.05]), 6, md=4)
    assert np.all(got["divergent"][0] == 1) and np.all(got["accept_prob"][0] == 0.0) and np.all(got["n_leapfrog"][0] == 1)
    assert np.array_equal(got["draws"][:, :, 0], np.repeat(x0[:, :1], 6, axis=1))                 # nothing non-finite entered the state
    assert np.all(got["logp"][0] == got["logp"][0, 0]) and np.isclose(got["logp"][0, 0], float(tg.logp(x0[:, 0])), rtol=1e-12, atol=0)
    assert np.all(np.isfinite(got["draws"])) and np.all(got["divergent"][1] == 0) and got["accept_prob"][1].mean() > 0.5
    xbad = x0.copy()
    xbad[3, 1] = np.inf
    eng.nuts_fused_enqueue([0, 0], xbad, seeds, 0.05, 4, 2)
    with pytest.raises(pfmi_mod.PfmiError) as ex:
        eng.nuts_wait()
    assert ex.value.code == -5 and "chain 1" in str(ex.value)                                     # PFMI_ERR_NUMERIC
    again = _plain(eng, [0, 0], x0, seeds, np.array([1e200, 0.05]), 6, md=4)                      # the ctx samples afterwards
    _same(got, again, "after a bad start")


def test_sampling_case_on_the_built_in_target(pfmi_mod, eng):
    tg, _, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(tg)
    eng.optimize_batch(pfmi_mod.HostRNG(3).rand(8).reshape(1, 8) * 4 - 2, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(8)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    got = _plain(eng, [0] * H.SAMPLING_K, X0, seeds, H.SAMPLING_EPS, 20, md=6)
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    print("NUTS_FUSED_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), got["accept_prob"].mean(), np.bincount(got["tree_depth"].ravel()))
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
    fin = C.c_int32()

    def args(k, pts, x, sd, eps):
        p = np.array(pts, dtype=np.int64)
        s = np.array(eps, dtype=np.float64)
        return (e.ctx, k, p.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp), None if sd is None else sd.ctypes.data_as(u64p),
                s.ctypes.data_as(dp))

    def enq(k=2, pts=(0, 0), x=x0, sd=seeds, eps=(0.1, 0.1), md=3, w=0, t=2, delta=0.8, flags=0):
        return L.pfmi_nuts_fused_enqueue(*args(k, pts, x, sd, eps), md, w, t, C.c_double(delta), flags)

    def hmc_fused(flags=0):
        return L.pfmi_hmc_fused_enqueue(*args(2, (0, 0), x0, seeds, (0.1, 0.1)), 2, 0, 2, C.c_double(0.8), flags)

    try:
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        assert enq() == -3 and b"pfmi_fit_batch" in L.pfmi_last_error()                 # PFMI_ERR_STATE: not fitted
        assert enq(k=0) == -3                                                           # ... which comes before the arguments
        e.fit_batch(6)
        for bad in (dict(k=0), dict(x=None), dict(sd=None), dict(md=0), dict(md=11), dict(t=0), dict(flags=4), dict(pts=(0, 10 ** 6)),
                    dict(pts=(-1, 0)), dict(eps=(0.1, 0.0)), dict(eps=(np.nan, 0.1)), dict(w=-1), dict(w=3, flags=1), dict(w=3, flags=2),
                    dict(w=3, delta=0.0), dict(w=3, delta=1.0)):
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG
            assert L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3            # ... which leaves no run behind
            assert L.pfmi_nuts_wait(e.ctx) == -3
        assert enq(md=0, flags=1) == -1                                                 # the sampler's parameter before what a CONTINUE needs
        assert enq(flags=1) == -3                                                       # PFMI_ERR_STATE: CONTINUE without chains
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0                              # the ctx is usable after the refusals
        assert L.pfmi_nuts_pump(e.ctx, C.byref(fin)) == 0 and fin.value == 1 and L.pfmi_hmc_wait(e.ctx) == -3
        r, n = C.c_int64(), C.c_int64()
        assert L.pfmi_nuts_stats(e.ctx, C.byref(r), C.byref(n)) == 0 and 3 <= r.value <= 15 and n.value == 0
        ptr, cnt = C.c_void_p(), C.c_int64()
        assert L.pfmi_hmc_draws_dev(e.ctx, C.byref(ptr), C.byref(cnt)) == 0 and ptr.value and cnt.value == 4
        assert L.pfmi_nuts_get_stats(e.ctx, None, None) == 0
        assert L.pfmi_nuts_get_path(e.ctx, 0, 1, None, None, None, None) == -3          # the run kept no path
        assert enq(flags=1) == 0 and enq(flags=1, k=1) == -3                            # CONTINUE with another K
        assert enq(flags=2) == 0 and L.pfmi_nuts_wait(e.ctx) == 0 and L.pfmi_nuts_stats(e.ctx, C.byref(r), None) == 0
        assert L.pfmi_nuts_get_path(e.ctx, 0, r.value, None, None, None, None) == 0     # the rows are the trips made ...
        assert L.pfmi_nuts_get_path(e.ctx, 0, r.value + 1, None, None, None, None) == -1           # ... and no more
        assert L.pfmi_hmc_get_path(e.ctx, 0, 1, None, None, None) == -3                 # ... and it is not static HMC's path
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0 and enq(flags=1, md=4) == -1  # CONTINUE beyond the chains' checkpoints
        assert L.pfmi_nuts_wait(e.ctx) == -3                                            # ... which left no chains behind
        assert enq(w=3) == 0 and L.pfmi_nuts_wait(e.ctx) == 0 and L.pfmi_adapt_get(e.ctx, None, None, None, None, None, None) == 0
        # the chains of another sampler, fused static HMC's included
        assert hmc_fused() == 0 and L.pfmi_hmc_wait(e.ctx) == 0
        assert enq(flags=1) == -3 and b"pfmi_hmc_enqueue" in L.pfmi_last_error()
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0 and hmc_fused(flags=1) == -3
        # a staged scale: the metric kernels are not fused
        scale = np.ones((2, d))
        assert L.pfmi_chain_scale_set(e.ctx, 2, scale.ctypes.data_as(dp)) == 0
        assert enq() == -4 and b"scale" in L.pfmi_last_error()
        assert L.pfmi_chain_scale_set(e.ctx, 0, None) == 0
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0
        # after the new runs, the existing enqueues still refuse the built-in target
        head = args(2, (0, 0), x0, seeds, (0.1, 0.1))
        assert L.pfmi_hmc_enqueue(*head, 2, 2, 0) == -4
        assert L.pfmi_nuts_enqueue(*head, 3, 2, 0) == -4
        assert L.pfmi_nuts_enqueue(*head, 3, 2, 1) == -4                                # ... a CONTINUE of the fused chains included
        assert L.pfmi_hmc_adapt_enqueue(*head, 2, 3, 2, C.c_double(0.8), 0) == -4
        assert L.pfmi_nuts_adapt_enqueue(*head, 3, 3, 2, C.c_double(0.8), 0) == -4
        assert L.pfmi_nuts_adapt_metric_enqueue(*head, 3, 3, 2, C.c_double(0.8), 0) == -4
        assert L.pfmi_chees_enqueue(e.ctx, 2, head[2], head[3], head[4], C.c_double(0.1), C.c_double(0.0), 8, 3, 2, C.c_double(0.651), 0) == -4
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0
        # any callback target: PFMI_ERR_UNSUPPORTED, with the entry point that serves it in the message; a change of target forgets the chains
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq() == -4 and b"pfmi_nuts_enqueue" in L.pfmi_last_error()
        assert L.pfmi_nuts_enqueue(*head, 3, 2, 1) == -3                                # no fused chains survive for the closure route
        e.set_target(tg)
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq(flags=1) == -3 and enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0
    finally:
        e.close()


def test_public_nuts_call_on_a_built_in_target(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(pfmi_mod.t_lowrank(20, r=2), 8, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        res = pfmi_mod.resample(res, 6, replace=False, rng=pfmi_mod.HostRNG(5))
        fixed = pfmi_mod.nuts(res, 12, step_size=0.2, max_depth=4, fused=True)
        assert isinstance(fixed, pfmi_mod.NUTSResult) and fixed.draws.shape == (20, 12, 6) and np.all(fixed.step_size == 0.2)
        assert np.all(fixed.tree_depth >= 1) and np.all(fixed.tree_depth <= 4) and np.all(fixed.n_leapfrog <= 15)
        assert e.nuts_stats() == (1 + int(np.max(np.sum(fixed.n_leapfrog, axis=1))), 0)
        win = pfmi_mod.nuts(res, 20, nwarmup=20, max_depth=6, rng=pfmi_mod.HostRNG(8), fused=True)
        dev = pfmi_mod.nuts(res, 20, nwarmup=20, max_depth=6, adapt="device", rng=pfmi_mod.HostRNG(8), fused=True)
        for out in (win, dev):
            assert isinstance(out, pfmi_mod.NUTSResult) and out.draws.shape == (20, 20, 6) and np.all(np.isfinite(out.draws))
            assert out.nwarmup == 20 and out.max_depth == 6
            for q in (out.logp, out.accept_prob, out.energy_error, out.divergent, out.tree_depth, out.n_leapfrog):
                assert q.shape == (6, 20)
            assert out.step_size.shape == (6,) and np.all(out.step_size > 0) and np.all(out.step_size != 20 ** -0.25)
            assert "chains: 6" in str(out) and "NUTS" in str(out) and "(warm-up: 20)" in str(out)
        assert win.warmup is None and dev.warmup["eps_trace"].shape == (6, 20) and dev.metric_scale is None
        s = dev.summary()                                              # served from the resident records
        assert s.nchains == 6 and s.ndraws == 20 and s.rhat.shape == (20,) and np.all(np.isfinite(s.mean)) and np.isfinite(s.lp["ess_bulk"])
        host = pfmi_mod.chain_diagnostics(dev.draws, e)
        assert np.array_equal(s.mean, host["mean"]) and np.array_equal(s.ess_bulk, host["ess_bulk"])
        with pytest.raises(ValueError, match="static HMC is available"):
            pfmi_mod.nuts(res, 5)
        with pytest.raises(ValueError, match="adapt_metric"):
            pfmi_mod.nuts(res, 5, nwarmup=30, adapt="device", adapt_metric=True, fused=True)
        with pytest.raises(ValueError, match="static HMC is available"):
            pfmi_mod.chees(res, 5)
    finally:
        e.close()


def test_fused_keyword_on_a_closure_target_raises(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        import torch
        tg = pfmi_mod.t_diag(10, 1)
        m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
        target = pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")
        res = pfmi_mod.multipathfinder(target, 6, nruns=2, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        with pytest.raises(ValueError, match="fused=True needs a built-in target"):
            pfmi_mod.nuts(res, 5, fused=True)
    finally:
        e.close()
