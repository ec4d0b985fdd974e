"""Device-resident warm-up (include/pfmi.h: pfmi_hmc_adapt_enqueue, pfmi_nuts_adapt_enqueue; the warm kernels of csrc/hmc_kernel.hip and
csrc/nuts_kernel.hip).  The main check needs no new trajectory checker: an adaptive run must be BIT-IDENTICAL to a host-driven replay of its
own step-size trace through the plain calls, whose arithmetic tests/test_gpu_hmc_steps.py and tests/test_gpu_nuts_steps.py pin.  The update
itself is checked against the long-double replay of tests/adapt_reference.py within the bound of tests/test_adapt_reference_cpu.py, which also
admits the sampling case on the float64 mirror."""
import ctypes as C

import numpy as np
import pytest

import adapt_reference as A
import hmc_reference as H
from helpers import demo_device_target, fit_seeds
from lbfgs_step_reference import HAVE_LONGDOUBLE, SKIP_REASON

pytestmark = pytest.mark.gpu

_ROWS = ("draws", "logp", "accept_prob", "energy_error", "divergent")
_DONE = {}                         # bit-equality case -> {"plans", "traces": (eps0, accept_trace, eps_trace, final step) per chain}: each case runs once


def _setup(pfmi_mod, eng, case):
    """the chains of tests/test_gpu_hmc_steps.py: metrics of a path's first point, an early point and its best fit; three step sizes"""
    d, J, tn = case[:3]
    eng.set_target(demo_device_target(H.grid_target(pfmi_mod, tn, d), grad=True))
    npts = eng.optimize_batch(H.grid_path_x0(pfmi_mod, tn, d), J, 40, 1e-8)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    P = int(npts[0])
    _, _, best = eng.elbo_batch(32, fit_seeds(P, 5))
    p_best = int(best[0])
    early = [p for p in range(1, P) if status[p] == 0 and 0 < jeff[p] < J]
    assert status[0] == 0 and early and status[p_best] == 0
    pts = np.array([0, early[0], p_best], dtype=np.int64)
    th, _, _ = eng.get_trace(0)
    x0 = np.asfortranarray(np.repeat(th[p_best][:, None], H.GRID_K, axis=1))
    return pts, x0, H.grid_eps(d), H.grid_seeds(d, J)


def _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T, pump=False):
    """one adaptive run: (rows, warm-up traces); NUTS rows carry tree_depth and n_leapfrog"""
    if sampler == "hmc":
        eng.hmc_adapt_enqueue(pts, x0, seeds, eps0, A.BIT_LF, W, T)
        eng.hmc_wait()
    else:
        eng.nuts_adapt_enqueue(pts, x0, seeds, eps0, A.BIT_DEPTH, W, T)
        if pump:
            for _ in range(1 + (W + T) * 2 ** A.BIT_DEPTH):
                if eng.nuts_pump():
                    break
                eng.sync()
        eng.nuts_wait()
    got = eng.hmc_get()
    if sampler == "nuts":
        got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got, eng.adapt_get()


def _plain(eng, sampler, pts, x0, seeds, eps, T, cont):
    if sampler == "hmc":
        eng.hmc_enqueue(pts, None if cont else x0, seeds, eps, A.BIT_LF, T, cont=cont)
        eng.hmc_wait()
    else:
        eng.nuts_enqueue(pts, None if cont else x0, seeds, eps, A.BIT_DEPTH, T, cont=cont)
        eng.nuts_wait()
    got = eng.hmc_get()
    if sampler == "nuts":
        got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got


def _replay_equals(eng, sampler, pts, x0, seeds, got, warm, W, T, label):
    """the run's own step-size trace through the plain calls: W calls of one transition, then one call of T"""
    for t in range(W):
        one = _plain(eng, sampler, pts, x0, seeds, warm["eps_trace"][:, t], 1, cont=t > 0)
        assert np.array_equal(one["accept_prob"][:, 0], warm["accept_trace"][:, t]), (label, t, one["accept_prob"][:, 0], warm["accept_trace"][:, t])
        assert np.array_equal(one["divergent"][:, 0], warm["divergent"][:, t]), (label, t)
        if sampler == "nuts":
            assert np.array_equal(one["n_leapfrog"][:, 0], warm["n_leapfrog"][:, t]), (label, t)
        else:
            assert np.all(warm["n_leapfrog"][:, t] == A.BIT_LF)
    last = _plain(eng, sampler, pts, x0, seeds, warm["step_size"], T, cont=True)
    for q in got:
        assert np.array_equal(last[q], got[q]), (label, q)


def _bit_case(pfmi_mod, eng, case):
    """runs one bit-equality case (both samplers) unless this session already has; returns its plans and traces"""
    if case in _DONE:
        return _DONE[case]
    out = {"plans": set(), "traces": []}
    d, J, tn, W, T = case
    kpad = H.kpad_for(J)
    route = "res" if H.resident(d, kpad) else "stream"
    pts, x0, eps0, seeds = _setup(pfmi_mod, eng, case)
    for sampler in ("hmc", "nuts"):
        plan = "%s_adapt:%d:%s" % (sampler, kpad, route)
        plain = "%s:%d:%s" % (sampler, kpad, route)
        before, pbefore = eng.kernel_time(plan)[1], eng.kernel_time(plain)[1]
        got, warm = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T)
        launches = eng.kernel_time(plan)[1] - before
        assert eng.kernel_time(plain)[1] == pbefore                      # the plain runs' counters are untouched
        if sampler == "hmc":
            assert launches == 1 + (W + T) * A.BIT_LF and eng.hmc_stats() == (launches, launches * H.GRID_K)
        else:
            assert 1 + (W + T) <= launches <= 1 + (W + T) * (2 ** A.BIT_DEPTH - 1)
        out["plans"].add(plan)
        assert got["draws"].shape == (d, T, H.GRID_K) and warm["eps_trace"].shape == (H.GRID_K, W)
        assert np.array_equal(warm["eps_trace"][:, 0], eps0) and np.all(warm["status"] == 0)
        assert np.all(np.isfinite(warm["eps_trace"])) and np.all(warm["eps_trace"] > 0) and np.all(warm["step_size"] > 0)
        for k in range(H.GRID_K):
            out["traces"].append((float(eps0[k]), warm["accept_trace"][k].copy(), warm["eps_trace"][k].copy(), float(warm["step_size"][k])))
        _replay_equals(eng, sampler, pts, x0, seeds, got, warm, W, T, (A.bit_case_id(case), sampler))
    _DONE[case] = out
    return out


@pytest.mark.parametrize("case", A.BIT_CASES, ids=[A.bit_case_id(c) for c in A.BIT_CASES])
def test_adaptive_run_is_bit_identical_to_its_replay_through_the_plain_calls(pfmi_mod, eng, case):
    assert len(_bit_case(pfmi_mod, eng, case)["traces"]) == 2 * H.GRID_K


def test_both_factor_routes_ran(pfmi_mod, eng):
    """the warm kernels were launched with the factor rows staged in LDS and streamed from HBM"""
    need = {"%s_adapt:%d:%s" % (s, H.kpad_for(c[1]), "res" if H.resident(c[0], H.kpad_for(c[1])) else "stream") for c in A.BIT_CASES
            for s in ("hmc", "nuts")}
    assert any(p.endswith(":res") for p in need) and any(p.endswith(":stream") for p in need)
    ran = set().union(*[_bit_case(pfmi_mod, eng, case)["plans"] for case in A.BIT_CASES])
    assert need <= ran, need - ran


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason=SKIP_REASON)
def test_device_update_matches_the_long_double_replay(pfmi_mod, eng):
    """from the recorded a_t, the long-double replay gives eps_trace[1:] and the final step size within the CPU test's bound"""
    traces = [t for case in A.BIT_CASES for t in _bit_case(pfmi_mod, eng, case)["traces"]]
    worst = 0.0
    for eps0, acc, trace, final in traces:
        be, bb, re, rb = A.bound(eps0, 0.8, acc)
        W = len(acc)
        q = [abs(float(A.LD(trace[m]) / re[m] - 1)) / be[m - 1] for m in range(1, W)] + [abs(float(A.LD(final) / rb[W - 1] - 1)) / bb[W - 1]]
        worst = max(worst, max(q))
    print("ADAPT_PARITY gpu chains", len(traces), "largest ratio", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_a_chain_does_not_depend_on_k_or_on_how_it_is_pumped(pfmi_mod, eng, sampler):
    case = (64, 6, "gauss", 6, 2)
    pts, x0, eps0, seeds = _setup(pfmi_mod, eng, case)
    got3, warm3 = _adaptive(eng, sampler, pts, x0, seeds, eps0, 6, 2)
    if sampler == "nuts":
        gotp, warmp = _adaptive(eng, sampler, pts, x0, seeds, eps0, 6, 2, pump=True)
        for q in got3:
            assert np.array_equal(gotp[q], got3[q]), q
        for q in warm3:
            assert np.array_equal(warmp[q], warm3[q]), q
    for k in range(H.GRID_K):
        got1, warm1 = _adaptive(eng, sampler, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps0[k:k + 1], 6, 2)
        assert np.array_equal(got1["draws"][:, :, 0], got3["draws"][:, :, k])
        for q in got3:
            if q != "draws":
                assert np.array_equal(got1[q][0], got3[q][k]), (k, q)
        for q in warm3:
            assert np.array_equal(warm1[q][0], warm3[q][k]), (k, q)


@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_divergent_warm_up(pfmi_mod, eng, sampler):
    """A funnel chain that starts at eps_0 = 1e200 beside a sane one, W = 8.  With a_t = 0 the update gives Hbar_m = delta m / (m + 10) and
    le_m = log(1e201) - 20 sqrt(m) delta m / (m + 10): every update lowers the step size, but from log(1e201) = 462.8 it takes until
    16 m^(3/2) / (m + 10) > 462.8, i.e. m = 857 transitions, to come down to 1 -- so all 8 warm-up transitions (and the sampling ones) of
    that chain are divergent, its updated step sizes fall strictly, and its state stays the start point."""
    W, T, d = 8, 2, 10
    tg = pfmi_mod.t_funnel(d)
    eng.set_target(demo_device_target(tg, grad=True))
    x = pfmi_mod.HostRNG(5).rand(2 * d).reshape(2, d) * 2 - 1
    eng.optimize_batch(x, 6, 40, 1e-8)
    eng.fit_batch(6)
    status, _, _, _ = eng.fit_status()
    assert status[0] == 0
    pts = np.array([0, 0], dtype=np.int64)
    x0 = np.asfortranarray(0.1 * np.ones((d, 2)))
    seeds = np.array([3, 4], dtype=np.uint64)
    eps0 = np.array([1e200, 0.05])
    m_down = next(m for m in range(1, 5000) if 16.0 * m ** 1.5 / (m + 10) > np.log(1e201))
    assert m_down == 857 and m_down > W
    got, warm = _adaptive(eng, sampler, pts, x0, seeds, eps0, W, T)
    one, warm1 = _adaptive(eng, sampler, pts[1:], x0[:, 1:], seeds[1:], eps0[1:], W, T)
    # the sane chain: finite throughout, the bits of the K = 1 run
    for q in got:
        assert np.all(np.isfinite(np.take(got[q], 1, axis=-1 if q == "draws" else 0))), q
        assert np.array_equal(np.take(one[q], 0, axis=-1 if q == "draws" else 0), np.take(got[q], 1, axis=-1 if q == "draws" else 0)), q
    for q in warm:
        assert np.all(np.isfinite(warm[q][1])) and np.array_equal(warm1[q][0], warm[q][1]), q
    assert warm["divergent"][1].sum() < W
    # the 1e200 chain
    assert np.all(warm["accept_trace"][0] == 0.0) and np.all(warm["divergent"][0] == 1)
    # (entry 0 is eps_0 itself; the updated steps exp(le_m), m = 1 .. W - 1, start at 10 eps_0 exp(-20 delta / 11) = 2.3 eps_0 and fall)
    assert warm["eps_trace"][0, 0] == 1e200 and np.all(np.diff(warm["eps_trace"][0, 1:]) < 0) and warm["eps_trace"][0, -1] > 1e190
    assert warm["status"][0] == 0
    ref, ref_bar = A.replay_ld(1e200, 0.8, np.zeros(W))[:2]
    assert np.allclose(warm["eps_trace"][0, 1:], np.asarray(ref[1:W], dtype=np.float64), rtol=1e-12, atol=0)
    assert np.isclose(warm["step_size"][0], float(ref_bar[W - 1]), rtol=1e-12, atol=0) and warm["step_size"][0] > 1e190
    assert np.all(got["divergent"][0] == 1) and np.all(got["accept_prob"][0] == 0.0)
    assert np.array_equal(got["draws"][:, :, 0], np.repeat(x0[:, :1], T, axis=1))          # the state never left the start point
    assert np.all(got["logp"][0] == got["logp"][0, 0]) and abs(got["logp"][0, 0] - tg.logp(x0[:, 0])) <= 1e-13


def test_chains_sample_the_target_after_the_device_warm_up(pfmi_mod, eng):
    """hmc_reference.sampling_case through pfmi_hmc_adapt_enqueue with the W and T admitted on the mirror (tests/test_adapt_reference_cpu.py)"""
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    eng.set_target(demo_device_target(tg, grad=True))
    x = pfmi_mod.HostRNG(5).rand(tg.d).reshape(1, tg.d) * 4 - 2
    eng.optimize_batch(x, 6, 40, 1e-8)
    eng.fit_batch(6)
    assert np.array_equal(eng.get_fit(0, 0)["alpha"], np.ones(eng.d)), "the first point's fit is not the identity the CPU mirror assumes"
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    eng.hmc_adapt_enqueue([0] * H.SAMPLING_K, X0, seeds, H.SAMPLING_EPS, H.SAMPLING_LF, A.SAMPLING_W, A.SAMPLING_T)
    eng.hmc_wait()
    got, warm = eng.hmc_get(), eng.adapt_get()
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    print("ADAPT_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), "accept", got["accept_prob"].mean(), "eps", warm["step_size"].min(),
          warm["step_size"].max(), "divergent warm-up transitions", int(warm["divergent"].sum()))
    assert got["divergent"].sum() == 0 and np.all(warm["status"] == 0)
    assert H.sampling_ok(mean, var), (mean, var)


def _windows_reference(pfmi_mod, eng, sampler, pts, x0, seeds, d, nwarmup, ndraws, param, window=10, delta=0.8):
    """the window route as it stood before adapt= existed, spelled out on the plain Engine calls"""
    from pfmi.hmc import dual_averaging_init, dual_averaging_update
    enq, wait = (eng.hmc_enqueue, eng.hmc_wait) if sampler == "hmc" else (eng.nuts_enqueue, eng.nuts_wait)
    eps = np.full(len(pts), d ** -0.25)
    state, done, first = dual_averaging_init(eps), 0, True
    while done < nwarmup:
        n = min(window, nwarmup - done)
        enq(pts, x0, seeds, eps, param, n, cont=not first)
        wait()
        first, done = False, done + n
        state, eps, ebar = dual_averaging_update(state, eng.hmc_get(draws=False)["accept_prob"].mean(axis=1), delta)
    eps = np.asarray(ebar, dtype=np.float64)
    enq(pts, x0, seeds, eps, param, ndraws, cont=True)
    wait()
    return eng.hmc_get(), eps


def test_public_calls(pfmi_mod):
    import torch
    tg = pfmi_mod.t_diag(10, 1)
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
    e = pfmi_mod.Engine(0)
    try:
        target = pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")
        res = pfmi_mod.multipathfinder(target, 6, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        for fn, cls, sampler, kw, param in ((pfmi_mod.hmc, pfmi_mod.HMCResult, "hmc", {}, 8), (pfmi_mod.nuts, pfmi_mod.NUTSResult, "nuts", {"max_depth": 5}, 5)):
            win = fn(res, 20, nwarmup=20, rng=pfmi_mod.HostRNG(8), **kw)
            assert win.warmup is None
            # adapt="windows" is the default and gives what the loop it always was gives
            seeds = pfmi_mod.HostRNG(8).rand_u64(6)
            ref, eps = _windows_reference(pfmi_mod, e, sampler, win.metric_points, np.asfortranarray(np.asarray(res.draws)[:, :6]), seeds, 10, 20, 20, param)
            assert np.array_equal(win.step_size, eps)
            for q in _ROWS:
                assert np.array_equal(getattr(win, q), ref[q]), q
            out = fn(res, 20, nwarmup=20, rng=pfmi_mod.HostRNG(8), adapt="device", **kw)
            assert isinstance(out, cls) and out.nwarmup == 20
            assert out.draws.shape == win.draws.shape == (10, 20, 6) and np.all(np.isfinite(out.draws))
            for q in ("logp", "accept_prob", "energy_error", "divergent"):
                assert getattr(out, q).shape == (6, 20)
            assert out.step_size.shape == (6,) and np.all(out.step_size > 0) and np.all(out.step_size != 10 ** -0.25)
            assert sorted(out.warmup) == ["accept_trace", "divergent", "eps_trace", "n_leapfrog", "status"]
            assert out.warmup["eps_trace"].shape == (6, 20) and np.all(out.warmup["eps_trace"][:, 0] == 10 ** -0.25)
            assert np.array_equal(out.metric_points, win.metric_points)
            if sampler == "nuts":
                assert out.tree_depth.shape == (6, 20) and out.n_leapfrog.shape == (6, 20) and out.max_depth == 5
            s_out, s_win = out.summary(), win.summary()
            assert s_out.nchains == s_win.nchains == 6 and s_out.ndraws == s_win.ndraws == 20 and s_out.rhat.shape == s_win.rhat.shape == (10,)
            assert np.all(np.isfinite(s_out.mean)) and "chains: 6" in str(out)
            with pytest.raises(ValueError, match="auto"):
                fn(res, 5, nwarmup=5, step_size=0.2, adapt="device", **kw)
            with pytest.raises(ValueError, match="nwarmup"):
                fn(res, 5, adapt="device", **kw)
            with pytest.raises(ValueError, match="windows"):
                fn(res, 5, adapt="host", **kw)
        # the positional construction of the results still works
        r = pfmi_mod.HMCResult(out.draws, out.logp, out.accept_prob, out.energy_error, out.divergent, out.step_size, out.metric_points, 3, 0, None, 0)
        assert r.warmup is None and r.nleapfrog == 3
    finally:
        e.close()


def test_return_codes_and_continue(pfmi_mod):
    from pfmi import _lib
    L = _lib.lib()
    d, K = 12, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
    seeds = np.array([1, 2], dtype=np.uint64)
    i64p, u64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

    def enq(fn, pts=(0, 0), x=x0, eps=(0.1, 0.1), param=2, W=3, T=2, delta=0.8, flags=0, k=K):
        pts = np.array(pts, dtype=np.int64)
        eps = np.array(eps, dtype=np.float64)
        return fn(e.ctx, k, pts.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp), seeds.ctypes.data_as(u64p), eps.ctypes.data_as(dp),
                  param, W, T, delta, flags)

    def adapt_get():
        return L.pfmi_adapt_get(e.ctx, None, None, None, None, None, None)

    try:
        with pytest.raises(pfmi_mod.PfmiError):
            e.adapt_get()
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        for fn in (L.pfmi_hmc_adapt_enqueue, L.pfmi_nuts_adapt_enqueue):
            assert enq(fn) == -3                                                        # PFMI_ERR_STATE: not fitted
        assert adapt_get() == -3
        e.fit_batch(6)
        P = e.P
        for fn, wait in ((L.pfmi_hmc_adapt_enqueue, L.pfmi_hmc_wait), (L.pfmi_nuts_adapt_enqueue, L.pfmi_nuts_wait)):
            for bad in (dict(flags=1), dict(flags=2), dict(flags=3), dict(flags=8), dict(W=0), dict(W=-1), dict(delta=0.0), dict(delta=1.0),
                        dict(delta=np.nan), dict(k=0), dict(pts=(0, P)), dict(eps=(0.1, 0.0)), dict(eps=(np.inf, 0.1)), dict(param=0), dict(T=0),
                        dict(x=None)):
                assert enq(fn, **bad) == -1, (fn, bad)                                  # PFMI_ERR_ARG
            assert adapt_get() == -3                                                    # no adaptive run so far / the refused ones left none
            assert enq(fn) == 0 and wait(e.ctx) == 0 and adapt_get() == 0
            for bad in (dict(flags=1), dict(W=0), dict(delta=1.0), dict(k=0)):          # a refused call of any kind leaves no chains and no traces
                assert enq(fn) == 0 and wait(e.ctx) == 0 and adapt_get() == 0
                assert enq(fn, **bad) == -1 and adapt_get() == -3, (fn, bad)
                assert L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3
        assert enq(L.pfmi_nuts_adapt_enqueue, param=11) == -1                           # max_depth outside 1 .. 10
        # a plain CONTINUE after an adaptive run goes on from W + T: the bits of one plain run of W + T + 3 transitions with the same steps
        W, T = 3, 2
        e.hmc_adapt_enqueue([0, 0], x0, seeds, [0.1, 0.1], 2, W, T)
        e.hmc_wait()
        warm = e.adapt_get()
        assert e.hmc_get()["logp"].shape == (K, T)
        e.hmc_enqueue([0, 0], None, seeds, warm["step_size"], 2, 3, cont=True)
        e.hmc_wait()
        tail = e.hmc_get()
        assert e.hmc_stats() == (3 * 2, 3 * 2 * K)
        e.hmc_enqueue([0, 0], None, seeds, [0.07, 0.09], 2, 1, cont=True)               # ... and one with step sizes of the caller's own
        e.hmc_wait()
        again = e.adapt_get()                                                           # the traces and the final step sizes outlive a CONTINUE
        for q in warm:
            assert np.array_equal(again[q], warm[q]), q
        for t in range(W):
            e.hmc_enqueue([0, 0], x0, seeds, warm["eps_trace"][:, t], 2, 1, cont=t > 0)
            e.hmc_wait()
        e.hmc_enqueue([0, 0], None, seeds, warm["step_size"], 2, T + 3, cont=True)
        e.hmc_wait()
        whole = e.hmc_get()
        for q in _ROWS:
            assert np.array_equal(np.take(whole[q], range(T, T + 3), axis=1), tail[q]), q
        with pytest.raises(pfmi_mod.PfmiError):                                         # a fresh plain run forgot the traces
            e.adapt_get()
        assert adapt_get() == -3
        # PFMI_ERR_UNSUPPORTED, as for the plain enqueues: device closures without a gradient, built-in targets
        for fn in (L.pfmi_hmc_adapt_enqueue, L.pfmi_nuts_adapt_enqueue):
            e.set_target(demo_device_target(tg))
            assert enq(fn) == -4 and b"gradient" in L.pfmi_last_error(), fn
            e.set_target(tg)
            assert enq(fn) == -4, fn
        # PFMI_ERR_NUMERIC, as for the plain enqueues: a start point with a non-finite gradient is reported by the wait
        e.set_target(demo_device_target(tg, grad=True))
        xbad = x0.copy()
        xbad[0, 1] = np.inf
        assert enq(L.pfmi_hmc_adapt_enqueue, x=xbad) == 0 and L.pfmi_hmc_wait(e.ctx) == -5 and adapt_get() == -3
    finally:
        e.close()
