"""GPU tests of the streaming pipeline for device closures with a gradient (pfmi_stream_enqueue on a DEVICE_CALLBACK target that carries a
value-and-gradient closure, pfmi_set_target_gradient): the closure optimiser's rounds (pf_lbc_step_kernel + the gradient closure) are the
producer, the fits run on the published positions and each segment's ELBO scan is the device-closure route (draw writer, value closure,
scatter).  Streamed must equal the packed route
    pfmi_optimize_batch ; pfmi_fit_batch ; pfmi_elbo_batch_enqueue ; pool ; PSIS
bit for bit for the HIP example closures of examples/device_logp; only the layout differs (trace point l of path k is slot k * (maxiters + 1) + l).
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from helpers import DEMO_LIB

pytestmark = pytest.mark.gpu


def grad_target(pfmi_mod, tg):
    """the example HIP closures for a built-in target `tg`: value closure + value-and-gradient closure"""
    pfmi_mod.lib()
    L = C.CDLL(DEMO_LIB)
    dp = C.POINTER(C.c_double)
    if tg.kind == 1:
        return pfmi_mod.DeviceCallbackTarget(tg.d, C.cast(L.pfx_funnel_logp, C.c_void_p).value, None, host=tg, keepalive=L,
                                             grad_fn=C.cast(L.pfx_funnel_logp_grad, C.c_void_p).value)
    L.pfx_gauss_create.restype = C.c_void_p
    L.pfx_gauss_create.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_double]
    h = L.pfx_gauss_create(tg.d, tg.r, tg.mean.ctypes.data_as(dp), tg.a.ctypes.data_as(dp),
                           tg.Wd.ctypes.data_as(dp) if tg.r else None, tg.G.ctypes.data_as(dp) if tg.r else None, tg.offset)
    assert h
    return pfmi_mod.DeviceCallbackTarget(tg.d, C.cast(L.pfx_gauss_logp, C.c_void_p).value, C.c_void_p(h), host=tg, keepalive=(L, h),
                                         grad_fn=C.cast(L.pfx_gauss_logp_grad, C.c_void_p).value)


def _results(pfmi, e, K, N_r, ndraws, fail=None):
    e.pool_build_best(N_r, fail)
    comm = pfmi.Comm.init_all([e])
    res, idx, draws = comm.psis_resample(ndraws, seed=9)
    status, jeff, logdet, nrej = e.fit_status()
    elbo, se, best = e.elbo_batch_wait()
    traces = [e.get_trace(k) for k in range(K)]
    _, lr = e.pool_get(draws=False)                                  # the pool's log importance ratios (PSIS input)
    p = int(e.offsets[0]) + int(best[0])
    fit = e.get_fit(p, int(jeff[p])) if best[0] > 0 else None
    out = dict(off=e.offsets.copy(), status=status, jeff=jeff, logdet=logdet, nrej=nrej, elbo=elbo, se=se, best=best, res=res, idx=idx,
               draws=draws, traces=traces, fit=fit, lr=lr)
    comm.close()
    return out


def _packed(pfmi, t, x0, J, maxiters, N, sd, N_r=64, ndraws=50):
    K = x0.shape[0]
    cap = maxiters + 1
    e = pfmi.Engine(0)
    try:
        e.set_target(t)
        npts = e.optimize_batch(x0, J, maxiters)
        e.fit_batch(J)
        seeds = np.concatenate([np.concatenate([[np.uint64(0)], sd[k * cap:k * cap + int(npts[k]) - 1]]) for k in range(K)]).astype(np.uint64)
        e.elbo_batch_enqueue(N, seeds)
        fail = np.array([sd[k * cap + int(npts[k]) - 1] for k in range(K)], dtype=np.uint64)
        out = _results(pfmi, e, K, N_r, ndraws, fail)
        out["npts"] = npts
        out["stats"] = e.optimize_stats()
        return out
    finally:
        e.close()


def _stream(pfmi, e, x0, J, maxiters, N, sd, N_r=64, ndraws=50):
    K = x0.shape[0]
    e.stream_enqueue(x0, N, sd, J, maxiters)
    npts = e.stream_wait()
    out = _results(pfmi, e, K, N_r, ndraws)
    out["npts"] = npts
    out["stats"] = e.optimize_stats()
    return out


def _streamed(pfmi, t, x0, J, maxiters, N, sd, repeat=1, **kw):
    e = pfmi.Engine(0)
    try:
        e.set_target(t)
        return [_stream(pfmi, e, x0, J, maxiters, N, sd, **kw) for _ in range(repeat)]
    finally:
        e.close()


def _compare(a, s, K, cap, exact=True):
    """a: packed route, s: streamed (fixed stride)"""
    np.testing.assert_array_equal(a["npts"], s["npts"])
    np.testing.assert_array_equal(a["nrej"], s["nrej"])
    for k in range(K):
        n = int(a["npts"][k])
        pa, ps = int(a["off"][k]), k * cap
        for name in ("status", "jeff", "logdet"):
            np.testing.assert_array_equal(a[name][pa:pa + n], s[name][ps:ps + n], err_msg=f"{name} path {k}")
        for name in ("elbo", "se"):
            if exact:
                np.testing.assert_array_equal(a[name][pa:pa + n], s[name][ps:ps + n], err_msg=f"{name} path {k}")
            else:
                np.testing.assert_allclose(a[name][pa:pa + n], s[name][ps:ps + n], rtol=1e-12, atol=0, err_msg=f"{name} path {k}")
        assert np.all(s["status"][ps + n:ps + cap] == 4), "slots a path never reached carry PFMI_FIT_ABSENT"
        assert np.all(np.isnan(s["elbo"][ps + n:ps + cap]))
        for i in range(3):
            np.testing.assert_array_equal(a["traces"][k][i], s["traces"][k][i])
    if not exact:
        return
    np.testing.assert_array_equal(a["best"], s["best"])
    np.testing.assert_array_equal(a["idx"], s["idx"])
    np.testing.assert_array_equal(a["draws"], s["draws"])
    np.testing.assert_equal(a["res"]["pareto_shape"], s["res"]["pareto_shape"])
    np.testing.assert_array_equal(a["lr"], s["lr"])
    assert a["res"]["tail_length"] == s["res"]["tail_length"]
    if a["fit"] is not None:
        for name in ("alpha", "B", "D", "qr_factors", "T", "V", "mu"):
            np.testing.assert_array_equal(a["fit"][name], s["fit"][name], err_msg=name)
        assert a["fit"]["logdet"] == s["fit"]["logdet"]


def _case(pfmi, kind, d, K, seed, scale=None):
    tg = pfmi.t_funnel(d) if kind == "funnel" else pfmi.t_lowrank(d, r=8, seed=2 + seed % 5)
    scale = scale or (10.0 if kind == "funnel" else 2.0)
    x0 = pfmi.HostRNG(100 + seed).rand(K * d).reshape(K, d) * 2 * scale - scale
    return tg, x0


def test_streamed_closure_equals_packed_random_shapes(pfmi_mod):
    """a dozen seeded shapes (low-rank Gaussian / funnel closures, K 1 3 8 12, d 7 64 1000 2300, J 1 6 10 16, N 16 100 300, maxiters small
    enough that some paths stop at it), streamed against packed, bit for bit; rounds and closure columns are counted on both routes"""
    rs = np.random.RandomState(20261015)
    stopped_at_cap = 0
    for it in range(12):
        d = int(rs.choice([7, 64, 1000, 2300]))
        J = int(rs.choice([1, 6, 10, 16]))
        K = int(rs.choice([1, 3, 8, 12]))
        maxiters = int(rs.choice([4, 12, 30, 80]))
        N = int(rs.choice([16, 100, 300]))
        kind = "funnel" if rs.randint(2) else "lr"
        tg, x0 = _case(pfmi_mod, kind, d, K, it)
        t = grad_target(pfmi_mod, tg)
        cap = maxiters + 1
        sd = pfmi_mod.hostrng.rand_u64(300 + it, np.arange(K * cap, dtype=np.uint64), 9)
        a = _packed(pfmi_mod, t, x0, J, maxiters, N, sd)
        s = _streamed(pfmi_mod, t, x0, J, maxiters, N, sd)[0]
        try:
            _compare(a, s, K, cap)
        except AssertionError as ex:
            raise AssertionError(f"shape {it}: {kind} d {d} J {J} K {K} maxiters {maxiters} N {N}: {ex}") from ex
        assert s["stats"][0] > 0 and s["stats"][1] == s["stats"][0] * K
        stopped_at_cap += int(np.sum(a["npts"] == cap))
    assert stopped_at_cap > 0, "no path stopped at maxiters"


def test_same_bits_under_every_segment_policy_and_publication_step(pfmi_mod, monkeypatch):
    """where the segments are cut (PFMI_STREAM_POLICY 0 / 1 / 2, PFMI_STREAM_PUB 4 / 32) changes nothing; the same context twice"""
    tg, x0 = _case(pfmi_mod, "lr", 300, 8, 1)
    t = grad_target(pfmi_mod, tg)
    J, maxiters, N = 6, 60, 100
    cap = maxiters + 1
    sd = pfmi_mod.hostrng.rand_u64(41, np.arange(8 * cap, dtype=np.uint64), 9)
    a = _packed(pfmi_mod, t, x0, J, maxiters, N, sd)
    for key, val in (("PFMI_STREAM_POLICY", "0"), ("PFMI_STREAM_POLICY", "1"), ("PFMI_STREAM_POLICY", "2"), ("PFMI_STREAM_PUB", "4"),
                     ("PFMI_STREAM_PUB", "32")):
        monkeypatch.setenv(key, val)
        try:
            for s in _streamed(pfmi_mod, t, x0, J, maxiters, N, sd, repeat=2):
                _compare(a, s, 8, cap)
        finally:
            monkeypatch.delenv(key)


def test_streamed_closure_beyond_the_builtin_dimension_limit(pfmi_mod):
    """d = 20 000: the built-in streaming optimiser stops at 16 384; the closure's round kernel walks memory"""
    tg, x0 = _case(pfmi_mod, "lr", 20000, 2, 3)
    t = grad_target(pfmi_mod, tg)
    J, maxiters, N = 6, 15, 32
    cap = maxiters + 1
    sd = pfmi_mod.hostrng.rand_u64(43, np.arange(2 * cap, dtype=np.uint64), 9)
    a = _packed(pfmi_mod, t, x0, J, maxiters, N, sd)
    s = _streamed(pfmi_mod, t, x0, J, maxiters, N, sd)[0]
    _compare(a, s, 2, cap)


def test_two_engines_pumped_in_turn_equal_one_engine(pfmi_mod):
    """two contexts streamed by one thread (each pump calls its own closures on its own streams) give the paths of one context"""
    tg, x0 = _case(pfmi_mod, "funnel", 50, 6, 4)
    t = grad_target(pfmi_mod, tg)
    J, maxiters, N = 6, 40, 64
    cap = maxiters + 1
    sd = pfmi_mod.hostrng.rand_u64(45, np.arange(6 * cap, dtype=np.uint64), 9)
    one = _streamed(pfmi_mod, t, x0, J, maxiters, N, sd)[0]
    e1, e2 = pfmi_mod.Engine(0), pfmi_mod.Engine(0)
    try:
        for e in (e1, e2):
            e.set_target(t)
        e1.stream_enqueue(x0[:4], N, sd[:4 * cap], J, maxiters)
        e2.stream_enqueue(x0[4:], N, sd[4 * cap:], J, maxiters)
        active = [e1, e2]
        while active:
            active = [e for e in active if not e.stream_pump()]
        n1, n2 = e1.stream_wait(), e2.stream_wait()
        np.testing.assert_array_equal(np.concatenate([n1, n2]), one["npts"])
        el = np.concatenate([e1.elbo_batch_wait()[0], e2.elbo_batch_wait()[0]])
        np.testing.assert_array_equal(el, one["elbo"])
        for k in range(6):
            got = e1.get_trace(k) if k < 4 else e2.get_trace(k - 4)
            for u, v in zip(got, one["traces"][k]):
                np.testing.assert_array_equal(u, v)
    finally:
        e1.close()
        e2.close()


def _public(pfmi_mod, t, inits, ntries, engine):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = pfmi_mod.multipathfinder(t, 300, init=[x.copy() for x in inits], ndraws_elbo=128, ntries=ntries, rng=pfmi_mod.HostRNG(6),
                                     engine=engine, maxiters=80)
    return (r.draws.copy(), r.draw_component_ids.copy(), r.psis_result.pareto_shape, [p.num_tries for p in r.pathfinder_results],
            [p.fit_iteration for p in r.pathfinder_results], [p.success for p in r.pathfinder_results],
            [len(p.optim_trace) for p in r.pathfinder_results], r.pathfinder_results[1].draws.copy())


def test_public_call_streamed_equals_packed_with_retries(pfmi_mod, monkeypatch):
    """pfmi.multipathfinder on a gradient closure streams (rounds counted); PFMI_NO_STREAM=1 forces the packed route.  A run that starts AT
    the optimum has no fit: retried with ntries = 3, failed with ntries = 1.  Same draws, component ids, k-hat, tries, fit iterations and
    success on both routes."""
    d = 40
    tg = pfmi_mod.t_diag(d, seed=3)
    t = grad_target(pfmi_mod, tg)
    rng0 = pfmi_mod.HostRNG(4)
    inits = [tg.mean.copy(), rng0.rand(d) * 4 - 2, rng0.rand(d) * 4 - 2, rng0.rand(d) * 4 - 2]
    e = pfmi_mod.Engine(0)
    try:
        for ntries in (3, 1):
            monkeypatch.delenv("PFMI_NO_STREAM", raising=False)
            s = _public(pfmi_mod, t, inits, ntries, e)
            assert e.optimize_stats()[1] > 0
            monkeypatch.setenv("PFMI_NO_STREAM", "1")
            p = _public(pfmi_mod, t, inits, ntries, e)
            monkeypatch.delenv("PFMI_NO_STREAM", raising=False)
            np.testing.assert_array_equal(s[0], p[0]); np.testing.assert_array_equal(s[1], p[1]); np.testing.assert_array_equal(s[7], p[7])
            np.testing.assert_equal(s[2], p[2])
            assert s[3:7] == p[3:7], (s[3:7], p[3:7])
            if ntries == 3:
                assert s[3][0] == 2 and all(s[5]), s[3:6]
            else:
                assert s[3][0] == 1 and not s[5][0] and s[4][0] == 0 and all(s[5][1:]), s[3:6]
    finally:
        e.close()


def _torch_diag(pfmi_mod, tg):
    import torch
    m = torch.tensor(tg.mean, device="cuda")
    a = torch.tensor(tg.a, device="cuda")
    return pfmi_mod.TorchDeviceTarget(tg.d, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), grad="autograd")


def test_torch_autograd_closure_streamed_against_packed(pfmi_mod):
    """TorchDeviceTarget(grad="autograd"): traces bit-identical between the routes, ELBO tables within 1e-12 relative (torch's row
    reductions may depend on the batch width the scan hands the closure)"""
    tg = pfmi_mod.t_diag(30, seed=2)
    t = _torch_diag(pfmi_mod, tg)
    K, J, maxiters, N = 5, 6, 50, 100
    cap = maxiters + 1
    x0 = pfmi_mod.HostRNG(12).rand(K * 30).reshape(K, 30) * 4 - 2
    sd = pfmi_mod.hostrng.rand_u64(47, np.arange(K * cap, dtype=np.uint64), 9)
    a = _packed(pfmi_mod, t, x0, J, maxiters, N, sd)
    s = _streamed(pfmi_mod, t, x0, J, maxiters, N, sd)[0]
    _compare(a, s, K, cap, exact=False)
    assert s["stats"][1] > 0


def _raising_target(pfmi_mod, tg, where, after):
    """a torch closure pair that raises once: in the gradient closure (an optimiser round) or in the value closure (a scan segment)"""
    import torch
    m = torch.tensor(tg.mean, device="cuda")
    a = torch.tensor(tg.a, device="cuda")
    calls = {"grad": 0, "value": 0}
    fn = lambda X: -0.5 * (((X - m) ** 2) * a).sum(1)

    def value(X):
        calls["value"] += 1
        if where == "value" and calls["value"] == after:
            raise KeyError("value closure failed")
        return fn(X)

    def vg(X):
        calls["grad"] += 1
        if where == "grad" and calls["grad"] == after:
            raise KeyError("gradient closure failed")
        return fn(X), -(X - m) * a

    return pfmi_mod.TorchDeviceTarget(tg.d, value, grad=vg)


@pytest.mark.parametrize("where,after", [("grad", 5), ("value", 1)])
def test_closure_that_raises_mid_stream_propagates_and_engine_recovers(pfmi_mod, where, after):
    tg = pfmi_mod.t_diag(20, seed=4)
    K, J, maxiters, N = 4, 6, 60, 64
    cap = maxiters + 1
    x0 = pfmi_mod.HostRNG(13).rand(K * 20).reshape(K, 20) * 4 - 2
    sd = pfmi_mod.hostrng.rand_u64(49, np.arange(K * cap, dtype=np.uint64), 9)
    e = pfmi_mod.Engine(0)
    try:
        e.set_target(_raising_target(pfmi_mod, tg, where, after))
        e.stream_enqueue(x0, N, sd, J, maxiters)
        with pytest.raises(KeyError):
            e.stream_wait()
        again = _stream(pfmi_mod, e, x0, J, maxiters, N, sd)            # the same engine, the same (now quiet) closure
    finally:
        e.close()
    fresh = _streamed(pfmi_mod, _raising_target(pfmi_mod, tg, "none", 0), x0, J, maxiters, N, sd)[0]
    _compare(fresh, again, K, cap, exact=False)


def test_public_call_propagates_a_closure_exception(pfmi_mod):
    """multipathfinder: a closure that raises inside stream_pump propagates; the engine's next call equals a fresh engine's"""
    tg = pfmi_mod.t_diag(12, seed=5)
    e = pfmi_mod.Engine(0)
    try:
        with pytest.raises(KeyError):
            pfmi_mod.multipathfinder(_raising_target(pfmi_mod, tg, "grad", 3), 100, nruns=3, ndraws_elbo=32, rng=pfmi_mod.HostRNG(3), engine=e)
        r1 = pfmi_mod.multipathfinder(_raising_target(pfmi_mod, tg, "none", 0), 100, nruns=3, ndraws_elbo=32, rng=pfmi_mod.HostRNG(3), engine=e)
    finally:
        e.close()
    r2 = pfmi_mod.multipathfinder(_raising_target(pfmi_mod, tg, "none", 0), 100, nruns=3, ndraws_elbo=32, rng=pfmi_mod.HostRNG(3))
    np.testing.assert_array_equal(r1.draws, r2.draws)


def test_stream_still_refuses_what_it_cannot_run(pfmi_mod):
    """a device closure without a gradient, J = 17 on a gradient closure and a host closure: PFMI_ERR_UNSUPPORTED (-4)"""
    tg = pfmi_mod.t_funnel(16)
    x0 = np.zeros((2, 16)) + 0.5
    sd = np.zeros(2 * 11, dtype=np.uint64)
    e = pfmi_mod.Engine(0)
    try:
        L = C.CDLL(DEMO_LIB)
        e.set_target(pfmi_mod.DeviceCallbackTarget(16, C.cast(L.pfx_funnel_logp, C.c_void_p).value, None, host=tg, keepalive=L))
        for t, J in ((None, 6), (grad_target(pfmi_mod, tg), 17), (pfmi_mod.CallbackTarget(16, lambda x: float(-0.5 * (x @ x))), 6)):
            if t is not None:
                e.set_target(t)
            with pytest.raises(pfmi_mod._lib.PfmiError) as ei:
                e.stream_enqueue(x0, 16, sd, J, 10)
            assert getattr(ei.value, "code", None) == -4
        e.set_target(grad_target(pfmi_mod, tg))                   # and the context still streams afterwards
        e.stream_enqueue(x0, 16, sd, 6, 10)
        assert np.all(e.stream_wait() >= 1)
    finally:
        e.close()
