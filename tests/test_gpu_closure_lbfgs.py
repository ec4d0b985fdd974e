"""Device L-BFGS for user closures (pfmi_set_target_gradient + rounds of lbfgs_closure_kernel.hip): the traces of a DEVICE_CALLBACK
target with a value-and-gradient closure against the CPU oracle's driver, determinism and independence of the paths, the pipeline
behind it, the Python routing and the failure paths."""
import ctypes as C

import numpy as np
import pytest

from helpers import DEMO_LIB, fit_seeds, oracle_target
from oracle import pf_oracle as po

pytestmark = pytest.mark.gpu


def grad_target(pfmi_mod, tg):
    """the example HIP closures of examples/device_logp for a built-in target `tg`: value closure + value-and-gradient closure"""
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


def _traces(eng, K):
    return [eng.get_trace(k) for k in range(K)]


def _check_against_oracle(tg, x0, J, maxit, tr, name):
    ot = oracle_target(tg)
    th, lp, gr = tr
    assert np.array_equal(th[0], x0)
    P, Lo, G = po.optimize_trace(ot, x0, J, maxit)
    n = min(len(P), len(th), 8)
    np.testing.assert_allclose(th[:n], P[:n], rtol=1e-9, atol=1e-10)
    for l in sorted({0, 1, len(th) // 2, len(th) - 1}):
        lpo, go = po.logp_grad(ot, th[l])
        assert abs(lpo - lp[l]) <= 1e-11 * max(1.0, abs(lpo))
        np.testing.assert_allclose(gr[l], go, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(go).max()))
    assert np.all(np.diff(lp) >= -1e-9 * np.maximum(1.0, np.abs(lp[1:])))
    if name != "funnel" and len(th) <= maxit:
        assert np.abs(gr[-1]).max() <= 1e-8
        np.testing.assert_allclose(th[-1], P[-1], atol=1e-5)


@pytest.mark.parametrize("name,d,J,maxit", [("iso", 100, 6, 200), ("diag", 300, 6, 1000), ("lr", 1000, 6, 1000), ("lr16", 500, 6, 1000),
                                             ("funnel", 50, 6, 60), ("lr", 200, 24, 1000), ("iso", 20000, 6, 100)])
def test_closure_lbfgs_traces_match_oracle_driver(pfmi_mod, eng, name, d, J, maxit):
    """same assertions as test_device_lbfgs_traces_match_oracle_driver; d = 20 000 is beyond the register kernel's 16 384, J = 24
    beyond its 16"""
    tg = {"iso": pfmi_mod.t_iso, "diag": lambda d: pfmi_mod.t_diag(d, 1), "lr": lambda d: pfmi_mod.t_lowrank(d, 8, 2),
          "lr16": lambda d: pfmi_mod.t_lowrank(d, 16, 3), "funnel": pfmi_mod.t_funnel}[name](d)
    K = 3
    x0 = pfmi_mod.HostRNG(3).rand(K * d).reshape(K, d) * 4 - 2
    eng.set_target(grad_target(pfmi_mod, tg))
    npts = eng.optimize_batch(x0, J, maxit)
    rounds, cols = eng.optimize_stats()
    assert 0 < rounds <= maxit * 55 + 1 and cols == rounds * K
    assert np.all(npts >= 2) and np.all(npts <= maxit + 1)
    for k, tr in enumerate(_traces(eng, K)):
        _check_against_oracle(tg, x0[k], J, maxit, tr, name)


def test_closure_lbfgs_rejected_pair_branch(pfmi_mod, eng, monkeypatch):
    """PFMI_LBFGS_REJECT_EVERY: every 3rd pair fails the curvature test, as the host driver's _reject_every.  (The hook is set through the
    environment, which the test process honours, as test_device_lbfgs_rejected_pairs_follow_the_host_driver does.)"""
    from pfmi.optimize import optimize_with_trace
    tg = pfmi_mod.t_lowrank(200, 8, 2)
    x0 = pfmi_mod.HostRNG(5).rand(2 * 200).reshape(2, 200) * 4 - 2
    eng.set_target(grad_target(pfmi_mod, tg))
    monkeypatch.setenv("PFMI_LBFGS_REJECT_EVERY", "3")
    eng.optimize_batch(x0, 6, 1000)
    monkeypatch.delenv("PFMI_LBFGS_REJECT_EVERY")
    for k in range(2):
        th, lp, gr = eng.get_trace(k)
        ref = optimize_with_trace(tg, x0[k], 6, 1000, _reject_every=3)
        n = min(len(th), len(ref.points), 8)
        np.testing.assert_allclose(th[:n], ref.points[:n], rtol=1e-9, atol=1e-10)
        assert np.abs(gr[-1]).max() <= 1e-8
        np.testing.assert_allclose(th[-1], ref.points[-1], atol=1e-5)


def test_closure_lbfgs_deterministic_and_independent_of_batch(pfmi_mod, eng):
    """path k's trace is bit-identical run to run, alone and inside a batch of 7, and with two engines pumped in turn"""
    tg = pfmi_mod.t_lowrank(300, 8, 2)
    K = 7
    x0 = pfmi_mod.HostRNG(21).rand(K * 300).reshape(K, 300) * 4 - 2
    t = grad_target(pfmi_mod, tg)
    eng.set_target(t)
    eng.optimize_batch(x0, 6)
    a = _traces(eng, K)
    eng.optimize_batch(x0, 6)
    b = _traces(eng, K)
    for ta, tb in zip(a, b):
        for u, v in zip(ta, tb):
            assert np.array_equal(u, v)
    eng.optimize_batch(x0[3:4], 6)
    alone = eng.get_trace(0)
    for u, v in zip(alone, a[3]):
        assert np.array_equal(u, v)
    e2 = pfmi_mod.Engine(0)
    try:
        e2.set_target(t)
        eng.optimize_batch_enqueue(x0[:4], 6)
        e2.optimize_batch_enqueue(x0[4:], 6)
        active = [eng, e2]
        while active:
            active = [e for e in active if not e.optimize_batch_pump()]
        eng.optimize_batch_wait()
        e2.optimize_batch_wait()
        for k in range(K):
            got = eng.get_trace(k) if k < 4 else e2.get_trace(k - 4)
            for u, v in zip(got, a[k]):
                assert np.array_equal(u, v)
    finally:
        e2.close()


def test_closure_traces_feed_fit_and_scan_like_uploaded_ones(pfmi_mod, eng):
    """traces made by the closure optimiser, fitted and scanned, give the ELBOs of the same traces downloaded and re-uploaded"""
    tg = pfmi_mod.t_lowrank(64, 8, 2)
    eng.set_target(grad_target(pfmi_mod, tg))
    x0 = pfmi_mod.HostRNG(7).rand(5 * 64).reshape(5, 64) * 4 - 2
    npts = eng.optimize_batch(x0, 6)
    seeds = fit_seeds(int(npts.sum()), 4)
    eng.fit_batch(6)
    e1, s1, b1 = eng.elbo_batch(200, seeds)
    traces = _traces(eng, 5)
    eng.set_traces([t[0] for t in traces], [t[2] for t in traces])
    eng.fit_batch(6)
    e2, s2, b2 = eng.elbo_batch(200, seeds)
    assert np.array_equal(e1, e2, equal_nan=True) and np.array_equal(b1, b2)


class _NoHost:
    calls = 0

    def logp(self, x): _NoHost.calls += 1; raise AssertionError("host twin called")
    grad = logp
    logp_and_grad = logp


def _torch_diag(pfmi_mod, tg, host=None):
    import torch
    m = torch.tensor(tg.mean, device="cuda")
    a = torch.tensor(tg.a, device="cuda")
    return pfmi_mod.TorchDeviceTarget(tg.d, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=host, grad="autograd")


def test_multipathfinder_torch_autograd_takes_device_route(pfmi_mod):
    """TorchDeviceTarget(grad="autograd") optimises on the device (closure columns > 0, host twin never called); agrees with the
    host-optimiser run of the same model within test_multipathfinder_device_and_host_optimizers_agree's tolerances, recovers the
    target moments and is deterministic under a fixed rng"""
    tg = pfmi_mod.t_diag(10, 1)
    e = pfmi_mod.Engine(0)
    try:
        _NoHost.calls = 0
        res = pfmi_mod.multipathfinder(_torch_diag(pfmi_mod, tg, _NoHost()), 4000, nruns=8, ndraws_elbo=100, ndraws_per_run=1000,
                                       rng=pfmi_mod.HostRNG(9), engine=e)
        assert _NoHost.calls == 0 and e.optimize_stats()[1] > 0
        host = pfmi_mod.multipathfinder(tg, 4000, nruns=8, ndraws_elbo=100, ndraws_per_run=1000, rng=pfmi_mod.HostRNG(9), optimizer="host")
        for r in (res, host):
            assert all(p.success for p in r.pathfinder_results)
            assert r.psis_result.pareto_shape < 0.7
        best = [np.array([max(x.value for x in p.elbo_estimates) for p in r.pathfinder_results]) for r in (res, host)]
        np.testing.assert_allclose(best[0], best[1], atol=0.5)
        sd = np.sqrt(1 / tg.a)
        assert np.all(np.abs(res.draws.mean(1) - tg.mean) < 0.15 * sd)
        assert np.all(np.abs(res.draws.std(1) / sd - 1) < 0.15)
        r1 = pfmi_mod.multipathfinder(_torch_diag(pfmi_mod, tg), 500, nruns=4, ndraws_elbo=50, rng=pfmi_mod.HostRNG(2), engine=e)
        r2 = pfmi_mod.multipathfinder(_torch_diag(pfmi_mod, tg), 500, nruns=4, ndraws_elbo=50, rng=pfmi_mod.HostRNG(2), engine=e)
        np.testing.assert_array_equal(r1.draws, r2.draws)
    finally:
        e.close()


class _BallHost:
    """logp = -|x - m|^2 / 2 whose gradient is NaN outside the ball |x| <= R (the host statement of the torch closure below)"""
    def __init__(self, m, R):
        self.m, self.R = m, R

    def logp_and_grad(self, x):
        g = -(x - self.m)
        if x @ x > self.R ** 2:
            g = g * np.nan
        return float(-0.5 * ((x - self.m) @ (x - self.m))), g


def test_closure_nonfinite_gradient_records_offending_point_and_stops(pfmi_mod, eng):
    import torch
    from pfmi.optimize import optimize_with_trace
    d, R = 8, 2.0
    m = np.full(d, 3.0)
    mt = torch.tensor(m, device="cuda")

    def vg(X):
        lp = -0.5 * ((X - mt) ** 2).sum(1)
        g = -(X - mt)
        out = (X * X).sum(1, keepdim=True) > R * R
        return lp, torch.where(out, torch.full_like(g, float("nan")), g)

    t = pfmi_mod.TorchDeviceTarget(d, lambda X: -0.5 * ((X - mt) ** 2).sum(1), grad=vg)
    eng.set_target(t)
    x0 = np.zeros((1, d))
    npts = eng.optimize_batch(x0, 6, 100)
    th, lp, gr = eng.get_trace(0)
    ref = optimize_with_trace(_BallHost(m, R), x0[0], 6, 100)
    assert npts[0] == len(ref.points) and npts[0] < 101
    np.testing.assert_allclose(th, ref.points, rtol=1e-12, atol=1e-14)
    assert not np.all(np.isfinite(gr[-1])) and th[-1] @ th[-1] > R * R


def test_closure_exception_propagates_and_engine_recovers(pfmi_mod, eng):
    import torch
    tg = pfmi_mod.t_iso(16)
    calls = [0]

    def vg(X):
        calls[0] += 1
        if calls[0] == 4:
            raise KeyError("closure failed")
        return -0.5 * (X * X).sum(1), -X

    eng.set_target(pfmi_mod.TorchDeviceTarget(16, lambda X: -0.5 * (X * X).sum(1), grad=vg))
    x0 = pfmi_mod.HostRNG(1).rand(3 * 16).reshape(3, 16) * 4 - 2
    with pytest.raises(KeyError):
        eng.optimize_batch(x0, 6)
    npts = eng.optimize_batch(x0, 6)                      # the same engine, a clean run
    assert np.all(npts >= 2)
    for k in range(3):
        _check_against_oracle(tg, x0[k], 6, 1000, eng.get_trace(k), "iso")
    del torch


def test_gradient_abi_rules(pfmi_mod, eng):
    """set_target_gradient on a built-in target: PFMI_ERR_ARG; set_target clears the gradient; without a gradient the device and host
    callback targets are still refused by optimize_batch (PFMI_ERR_UNSUPPORTED)"""
    L = eng.L
    tg = pfmi_mod.t_iso(8)
    eng.set_target(tg)
    fn = C.cast(C.CDLL(DEMO_LIB).pfx_funnel_logp_grad, C.c_void_p)
    assert L.pfmi_set_target_gradient(eng.ctx, fn, None) == -1
    x0 = np.zeros((1, 8)) + 0.5
    npts = np.empty(1, dtype=np.int64)
    dp = C.POINTER(C.c_double)
    call = lambda: L.pfmi_optimize_batch(eng.ctx, C.c_int32(1), x0.ctypes.data_as(dp), C.c_int32(6), C.c_int32(100), C.c_double(1e-8),
                                         npts.ctypes.data_as(C.POINTER(C.c_int64)))
    t = grad_target(pfmi_mod, pfmi_mod.t_funnel(8))
    eng.set_target(t)
    assert call() == 0
    desc = t.descriptor()
    assert L.pfmi_set_target(eng.ctx, C.byref(desc)) == 0          # no gradient attached any more
    assert call() == -4
    eng.set_target(pfmi_mod.CallbackTarget(8, lambda x: -0.5 * float(x @ x)))
    assert call() == -4
