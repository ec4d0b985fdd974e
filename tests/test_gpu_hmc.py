"""Static HMC with the fitted Woodbury metric (pfmi_hmc_enqueue, pfmi.hmc) on the GPU: independence of a chain from K, continuation,
divergence handling, the integrator's order, the stationary distribution, the public call and every return code of the C ABI.  The
per-round arithmetic is pinned by tests/test_gpu_hmc_steps.py; the sampling and energy-order cases are shown on the float64 mirror,
with these seeds, by tests/test_hmc_reference_cpu.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import hmc_reference as H
from helpers import demo_device_target

pytestmark = pytest.mark.gpu

_KEYS = ("draws", "logp", "accept_prob", "energy_error", "divergent")


def _fitted(pfmi_mod, eng, tg, J=6, K=2, seed=5, scale=2.0, maxiters=40):
    """K closure-optimised paths on the example closure of `tg`, fitted; returns (status, j_eff, offsets)"""
    eng.set_target(demo_device_target(tg, grad=True))
    x0 = pfmi_mod.HostRNG(seed).rand(K * tg.d).reshape(K, tg.d) * 2 * scale - scale
    eng.optimize_batch(x0, J, maxiters, 1e-8)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    return status, jeff, eng.offsets


def _run(eng, pts, x0, seeds, eps, Lf, T, **kw):
    eng.hmc_enqueue(pts, x0, seeds, eps, Lf, T, **kw)
    eng.hmc_wait()
    return eng.hmc_get()


@pytest.fixture(scope="module")
def small(pfmi_mod, eng):
    """d = 20, J = 6, two paths: four chains on the first point (j_eff = 0), an early point and the last points of both paths"""
    tg = pfmi_mod.t_lowrank(20, r=2, seed=2, wscale=0.5)
    status, jeff, off = _fitted(pfmi_mod, eng, tg)
    pts = np.array([0, 2, off[1] - 1, off[2] - 1], dtype=np.int64)
    assert np.all(status[pts] == 0) and jeff[0] == 0 and 0 < jeff[2] < 6 and jeff[off[1] - 1] > jeff[2]
    x0 = np.asfortranarray(tg.mean[:, None] + 0.3 * np.random.default_rng(1).standard_normal((20, 4)))
    seeds = np.asarray(pfmi_mod.hostrng.rand_u64(31, np.arange(4, dtype=np.uint64), 9), dtype=np.uint64)
    return tg, pts, x0, seeds, np.array([0.2, 0.3, 0.25, 0.35])


def test_chain_does_not_depend_on_k(eng, small):
    """chain outputs at K = 1 are bit-identical to the same chain inside K = 4"""
    tg, pts, x0, seeds, eps = small
    all4 = _run(eng, pts, x0, seeds, eps, 3, 5)
    assert 0 < all4["accept_prob"].mean() <= 1 and np.all(np.isfinite(all4["draws"]))
    for k in range(4):
        one = _run(eng, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps[k:k + 1], 3, 5)
        assert np.array_equal(one["draws"][:, :, 0], all4["draws"][:, :, k])
        for q in _KEYS[1:]:
            assert np.array_equal(one[q][0], all4[q][k]), (k, q)


def test_continue_is_bit_identical_to_one_call(eng, small):
    """T = 6 in one call == 3 + PFMI_HMC_CONTINUE 3"""
    tg, pts, x0, seeds, eps = small
    whole = _run(eng, pts, x0, seeds, eps, 3, 6)
    a = _run(eng, pts, x0, seeds, eps, 3, 3)
    b = _run(eng, pts, None, seeds, eps, 3, 3, cont=True)
    assert eng.hmc_stats() == (3 * 3, 3 * 3 * 4)                      # no start evaluation: the states are resident
    assert np.array_equal(np.concatenate([a["draws"], b["draws"]], axis=1), whole["draws"])
    for q in _KEYS[1:]:
        assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), whole[q]), q


def test_divergent_transitions_leave_the_state_alone(pfmi_mod, eng):
    """a step so large that the funnel closure returns non-finite values: a = 0, divergent = 1, the state unchanged, every record finite"""
    tg = pfmi_mod.t_funnel(10)
    status, jeff, off = _fitted(pfmi_mod, eng, tg, scale=1.0)
    assert status[0] == 0
    x0 = np.asfortranarray(0.1 * np.ones((10, 2)))
    seeds = np.array([3, 4], dtype=np.uint64)
    got = _run(eng, [0, 0], x0, seeds, [1e200, 0.05], 3, 4)
    assert np.all(got["divergent"][0] == 1) and np.all(got["accept_prob"][0] == 0.0)
    assert np.array_equal(got["draws"][:, :, 0], np.repeat(x0[:, :1], 4, axis=1))
    assert np.all(got["logp"][0] == got["logp"][0, 0]) and abs(got["logp"][0, 0] - tg.logp(x0[:, 0])) <= 1e-13     # the start's own value
    for q in _KEYS:
        assert np.all(np.isfinite(got[q])), q
    assert np.all(got["divergent"][1] == 0) and got["accept_prob"][1].mean() > 0.5     # the sane chain beside it is untouched


def _identity_point(eng):
    f = eng.get_fit(0, 0)
    assert np.array_equal(f["alpha"], np.ones(eng.d)), "the first point's fit is not the identity the CPU mirror assumes"
    return 0


def test_energy_error_is_second_order(pfmi_mod, eng):
    """same starts and momenta, (e, Lf) = (0.1, 4) against (0.05, 8): max |H1 - H0| shrinks by 4 + O(e^2)"""
    tg, M, x0, seeds = H.energy_case(pfmi_mod)
    _fitted(pfmi_mod, eng, tg, K=1)
    p = _identity_point(eng)
    mx = [np.max(np.abs(_run(eng, [p] * H.ENERGY_K, x0, seeds, eps, Lf, 1)["energy_error"])) for eps, Lf in H.ENERGY_RUNS]
    ratio = mx[0] / mx[1]
    print("HMC_ENERGY_ORDER gpu", mx, ratio)
    assert H.ENERGY_RATIO[0] <= ratio <= H.ENERGY_RATIO[1], (mx, ratio)


def test_chains_sample_the_target(pfmi_mod, eng):
    """t_lowrank(8, r = 2) as a closure: 256 chains from 3 standard deviations off the mean, T = 60, Lf = 4, fixed step; the final states
    whitened with the target's true covariance have coordinate means within 5 / sqrt(256) and variances within 1 +- 5 sqrt(2 / 255)"""
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    _fitted(pfmi_mod, eng, tg, K=1)
    p = _identity_point(eng)
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    got = _run(eng, [p] * H.SAMPLING_K, X0, seeds, H.SAMPLING_EPS, H.SAMPLING_LF, H.SAMPLING_T)
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    print("HMC_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), got["accept_prob"].mean())
    assert got["divergent"].sum() == 0
    assert H.sampling_ok(mean, var), (mean, var)


def test_public_hmc_call(pfmi_mod):
    import torch
    tg = pfmi_mod.t_diag(10, 1)
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")

    def target():
        return pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")

    e, e2 = pfmi_mod.Engine(0), pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(target(), 6, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        out = pfmi_mod.hmc(res, 20, nwarmup=20, rng=pfmi_mod.HostRNG(8))
        assert isinstance(out, pfmi_mod.HMCResult)
        assert out.draws.shape == (10, 20, 6) and np.all(np.isfinite(out.draws))
        for q in (out.logp, out.accept_prob, out.energy_error, out.divergent):
            assert q.shape == (6, 20)
        assert out.step_size.shape == (6,) and np.all(out.step_size > 0) and np.all(out.step_size != 10 ** -0.25)
        pts = {r.fit_distribution.point for r in res.pathfinder_results}
        assert out.metric_points.shape == (6,) and set(out.metric_points.tolist()) <= pts
        assert "chains: 6" in str(out) and "Static HMC" in str(out)
        fixed = pfmi_mod.hmc(res, 5, nchains=2, step_size=0.2, nleapfrog=4)
        assert fixed.draws.shape == (10, 5, 2) and np.all(fixed.step_size == 0.2)
        single = pfmi_mod.hmc(res.pathfinder_results[0], 3, nchains=2, step_size=0.2)
        assert single.draws.shape == (10, 3, 2)
        with pytest.raises(ValueError, match="one engine"):                # a result sharded over two engines
            pfmi_mod.hmc(dataclasses.replace(res, engines=[e, e2]), 5)
        e.fit_batch(6)                                                   # a refit: the result's fit token is stale
        with pytest.raises(pfmi_mod.StaleHandleError):
            pfmi_mod.hmc(res, 5)
    finally:
        e.close()
        e2.close()


def test_return_codes(pfmi_mod):
    """every return code of pfmi_hmc_* through the C ABI; the ctx stays usable afterwards"""
    from pfmi import _lib
    L = _lib.lib()
    i64p, u64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    d, K = 12, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
    seeds = np.array([1, 2], dtype=np.uint64)

    def enq(pts=(0, 0), x=x0, sd=seeds, eps=(0.1, 0.1), Lf=2, T=2, flags=0, k=K):
        pts = np.array(pts, dtype=np.int64)
        eps = np.array(eps, dtype=np.float64)
        return L.pfmi_hmc_enqueue(e.ctx, k, pts.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp),
                                  None if sd is None else sd.ctypes.data_as(u64p), eps.ctypes.data_as(dp), Lf, T, flags)

    try:
        with pytest.raises(pfmi_mod.PfmiError, match="no hmc_enqueue"):                 # the wrapper before any run: the library's kind of error
            e.hmc_get()
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        with pytest.raises(pfmi_mod.PfmiError):                                         # a refused enqueue (not fitted) leaves no run behind
            e.hmc_enqueue([0, 0], x0, seeds, 0.1, 2, 2)
        with pytest.raises(pfmi_mod.PfmiError, match="no hmc_enqueue"):
            e.hmc_path()
        assert enq() == -3 and b"fit_batch" in L.pfmi_last_error()                    # PFMI_ERR_STATE: not fitted
        assert L.pfmi_hmc_wait(e.ctx) == -3 and L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3
        e.fit_batch(6)
        assert enq(flags=1) == -3                                                       # CONTINUE without a run
        assert L.pfmi_hmc_get_path(e.ctx, 0, 1, None, None, None) == -3
        P = e.P
        for bad in (dict(k=0), dict(pts=(0, P)), dict(pts=(-1, 0)), dict(eps=(0.1, 0.0)), dict(eps=(0.1, np.inf)), dict(eps=(np.nan, 0.1)),
                    dict(Lf=0), dict(T=0), dict(x=None), dict(sd=None), dict(flags=8)):
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG
        assert enq() == 0 and L.pfmi_hmc_wait(e.ctx) == 0                               # the ctx is usable after the refusals
        r, n = C.c_int64(), C.c_int64()
        assert L.pfmi_hmc_stats(e.ctx, C.byref(r), C.byref(n)) == 0 and (r.value, n.value) == (5, 10)
        ptr, cnt = C.c_void_p(), C.c_int64()
        assert L.pfmi_hmc_draws_dev(e.ctx, C.byref(ptr), C.byref(cnt)) == 0 and ptr.value and cnt.value == 4
        assert L.pfmi_hmc_get_path(e.ctx, 0, 1, None, None, None) == -3                 # the run kept no path
        assert enq(flags=1) == 0 and enq(flags=1, k=1) == -3                            # CONTINUE with another K
        # a new fit, the optimiser and a new target forget the chains
        assert enq() == 0
        e.fit_batch(6)
        assert L.pfmi_hmc_get(e.ctx, None, None, None, None, None) == -3 and enq(flags=1) == -3
        # PFMI_ERR_UNSUPPORTED: built-in targets, device closures without a gradient
        e.set_target(demo_device_target(tg))
        assert enq() == -4 and b"gradient" in L.pfmi_last_error()
        e.set_target(tg)
        assert enq() == -4
        # PFMI_ERR_NUMERIC: a point whose fit failed (negative-curvature pairs accepted: non-PD fits)
        rng = np.random.default_rng(0)
        e.set_target(demo_device_target(tg, grad=True))
        e.set_traces([np.cumsum(rng.normal(size=(9, d)), 0)], [rng.normal(size=(9, d))])
        e.fit_batch(5, -1e300)
        status = e.fit_status()[0]
        badp = int(np.flatnonzero(status != 0)[0])
        assert enq(pts=(0, badp)) == -5 and b"status" in L.pfmi_last_error()
        # a start point with a non-finite gradient is reported by the wait
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        xbad = x0.copy()
        xbad[0, 1] = np.inf
        assert enq(x=xbad) == 0 and L.pfmi_hmc_wait(e.ctx) == -5
        got = _run(e, [0, 0], x0, seeds, 0.1, 2, 3)                                      # ... and the ctx still samples
        assert np.all(np.isfinite(got["draws"]))
    finally:
        e.close()
