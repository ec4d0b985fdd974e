"""NUTS with the fitted Woodbury metric (pfmi_nuts_enqueue, pfmi.nuts) on the GPU: independence of a chain from K and from the pumping,
continuation, the round count, the trees against the float64 mirror, the shared records, the stationary distribution, the public call and
every return code of the C ABI.  The per-round arithmetic and every decision are pinned by tests/test_gpu_nuts_steps.py."""
import ctypes as C

import numpy as np
import pytest

import hmc_reference as H
import nuts_reference as N
from helpers import demo_device_target

pytestmark = pytest.mark.gpu

_KEYS = ("draws", "logp", "accept_prob", "energy_error", "divergent", "tree_depth", "n_leapfrog")


def _fitted(pfmi_mod, eng, tg, J=6, K=2, seed=5, scale=2.0, maxiters=40):
    eng.set_target(demo_device_target(tg, grad=True))
    x0 = pfmi_mod.HostRNG(seed).rand(K * tg.d).reshape(K, tg.d) * 2 * scale - scale
    eng.optimize_batch(x0, J, maxiters, 1e-8)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    return status, jeff, eng.offsets


def _get(eng):
    got = eng.hmc_get()
    got["tree_depth"], got["n_leapfrog"] = eng.nuts_get_stats()
    return got


def _run(eng, pts, x0, seeds, eps, md, T, pump=False, **kw):
    eng.nuts_enqueue(pts, x0, seeds, eps, md, T, **kw)
    if pump:
        passes = 0
        while not eng.nuts_pump():
            eng.sync()                                                   # one pass per round at the least: the window never fills
            passes += 1
            assert passes <= 1 + T * (2 ** md - 1), passes
    eng.nuts_wait()
    return _get(eng)


@pytest.fixture(scope="module")
def small(pfmi_mod, eng):
    """d = 20, J = 6, two paths: five chains on the first point (j_eff = 0), an early point and later points, at step sizes that give
    trees of different sizes"""
    tg = pfmi_mod.t_lowrank(20, r=2, seed=2, wscale=0.5)
    status, jeff, off = _fitted(pfmi_mod, eng, tg)
    pts = np.array([0, 2, off[1] - 1, off[2] - 1, off[1] - 1], dtype=np.int64)
    assert np.all(status[pts] == 0) and jeff[0] == 0 and 0 < jeff[2] < 6 and jeff[off[1] - 1] > jeff[2]
    x0 = np.asfortranarray(tg.mean[:, None] + 0.3 * np.random.default_rng(1).standard_normal((20, 5)))
    seeds = np.asarray(pfmi_mod.hostrng.rand_u64(31, np.arange(5, dtype=np.uint64), 9), dtype=np.uint64)
    return tg, pts, x0, seeds, np.array([0.05, 0.3, 0.1, 0.6, 0.02])


def _same(a, b, ka, kb):
    assert np.array_equal(a["draws"][:, :, ka], b["draws"][:, :, kb])
    for q in _KEYS[1:]:
        assert np.array_equal(a[q][ka], b[q][kb]), q


def test_chain_does_not_depend_on_k(eng, small):
    """chain outputs at K = 1 are bit-identical to the same chain inside K = 5, whose trees differ in size"""
    tg, pts, x0, seeds, eps = small
    all5 = _run(eng, pts, x0, seeds, eps, 6, 4)
    assert np.all(np.isfinite(all5["draws"])) and len(set(all5["n_leapfrog"].sum(axis=1).tolist())) > 1, all5["n_leapfrog"]
    assert np.all(all5["n_leapfrog"] >= 1) and np.all(all5["n_leapfrog"] <= 63) and np.all(all5["tree_depth"] <= 6)
    for k in range(5):
        one = _run(eng, pts[k:k + 1], x0[:, k:k + 1], seeds[k:k + 1], eps[k:k + 1], 6, 4)
        _same(one, all5, 0, k)


def test_continue_is_bit_identical_to_one_call(eng, small):
    """T = 6 in one call == 3 + 3 == 2 + 4 with PFMI_NUTS_CONTINUE"""
    tg, pts, x0, seeds, eps = small
    whole = _run(eng, pts, x0, seeds, eps, 5, 6)
    for first in (3, 2):
        a = _run(eng, pts, x0, seeds, eps, 5, first)
        b = _run(eng, pts, None, seeds, eps, 5, 6 - first, cont=True)
        assert eng.nuts_stats()[0] == int(np.max(b["n_leapfrog"].sum(axis=1)))          # no start evaluation: the states are resident
        for q in _KEYS:
            assert np.array_equal(np.concatenate([a[q], b[q]], axis=1), whole[q]), (first, q)


def test_pumping_round_by_round_is_bit_identical_to_wait(eng, small):
    tg, pts, x0, seeds, eps = small
    a = _run(eng, pts, x0, seeds, eps, 5, 4)
    b = _run(eng, pts, x0, seeds, eps, 5, 4, pump=True)
    for q in _KEYS:
        assert np.array_equal(a[q], b[q]), q


def test_rounds_and_trees_equal_the_mirror(pfmi_mod, eng, small):
    """rounds == 1 + max_k sum_t n_leapfrog[k, t]; on this well-conditioned case every tree's depth and leaf count are the float64
    mirror's integers (the factors of the chains' fits, the chains' seeds)"""
    tg, pts, x0, seeds, eps = small
    got = _run(eng, pts, x0, seeds, eps, 6, 5)
    rounds, columns = eng.nuts_stats()
    assert rounds == 1 + int(np.max(got["n_leapfrog"].sum(axis=1)))
    assert columns % 5 == 0 and rounds <= columns // 5 <= rounds + 4
    jeff = eng.fit_status()[1]
    for k in range(5):
        p = int(pts[k])
        M = H.Metric.from_fit(eng.get_fit(p, int(jeff[p])))
        rec = N.mirror(M, tg.logp_and_grad, x0[:, k], int(seeds[k]), float(eps[k]), 6, 5)
        assert np.array_equal(rec["tree_depth"], got["tree_depth"][k]) and np.array_equal(rec["n_leapfrog"], got["n_leapfrog"][k]), k
        assert np.array_equal(rec["divergent"], got["divergent"][k])
        assert np.allclose(rec["draws"].T, got["draws"][:, :, k], rtol=1e-9, atol=1e-9)


def test_shared_records_serve_a_nuts_run(pfmi_mod, eng, small):
    """pfmi_hmc_get, the device pointer and the resident chain diagnostics on a NUTS run; CONTINUE of one kind on the other kind's chains"""
    tg, pts, x0, seeds, eps = small
    got = _run(eng, pts, x0, seeds, eps, 5, 16)
    res = eng.chain_diagnostics(with_lp=True)
    host = eng.chain_diagnostics(got["draws"])
    for q in eng.CHAIN_KEYS:
        assert np.array_equal(res[q][:20], host[q]), q
    assert np.all(got["accept_prob"] > 0) and np.all(got["accept_prob"] <= 1)
    with pytest.raises(pfmi_mod.PfmiError) as ex:
        eng.hmc_enqueue(pts, None, seeds, eps, 3, 2, cont=True)
    assert ex.value.code == -3
    eng.hmc_enqueue(pts, x0, seeds, eps, 3, 2)
    eng.hmc_wait()
    with pytest.raises(pfmi_mod.PfmiError) as ex:
        eng.nuts_enqueue(pts, None, seeds, eps, 5, 2, cont=True)
    assert ex.value.code == -3


def test_chains_sample_the_target(pfmi_mod, eng):
    """hmc_reference.sampling_case: 256 chains from 3 standard deviations off the mean; the final states whitened with the target's true
    covariance within hmc_reference.sampling_ok's bounds"""
    tg, M, x0, seeds, Lc = H.sampling_case(pfmi_mod)
    _fitted(pfmi_mod, eng, tg, K=1)
    f = eng.get_fit(0, 0)
    assert np.array_equal(f["alpha"], np.ones(eng.d))
    X0 = np.asfortranarray(np.repeat(x0[:, None], H.SAMPLING_K, axis=1))
    got = _run(eng, [0] * H.SAMPLING_K, X0, seeds, H.SAMPLING_EPS, 6, 20)
    mean, var = H.sampling_stats(tg, Lc, got["draws"][:, -1, :])
    print("NUTS_SAMPLING gpu", np.max(np.abs(mean)), np.min(var), np.max(var), got["accept_prob"].mean(), np.bincount(got["tree_depth"].ravel()))
    assert got["divergent"].sum() == 0
    assert H.sampling_ok(mean, var), (mean, var)


def test_public_nuts_call(pfmi_mod):
    import torch
    tg = pfmi_mod.t_diag(10, 1)
    m, a = torch.tensor(tg.mean, device="cuda"), torch.tensor(tg.a, device="cuda")
    target = pfmi_mod.TorchDeviceTarget(10, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg, grad="autograd")
    e = pfmi_mod.Engine(0)
    try:
        res = pfmi_mod.multipathfinder(target, 6, nruns=3, ndraws_elbo=20, ndraws_per_run=20, rng=pfmi_mod.HostRNG(4), engine=e)
        # six windows of dual averaging: the first update steps to 10 times the initial step size, as Hoffman & Gelman's rule does
        out = pfmi_mod.nuts(res, 40, nwarmup=60, max_depth=6, rng=pfmi_mod.HostRNG(8))
        assert isinstance(out, pfmi_mod.NUTSResult) and isinstance(out, pfmi_mod.HMCResult)
        assert out.draws.shape == (10, 40, 6) and np.all(np.isfinite(out.draws))
        for q in (out.logp, out.accept_prob, out.energy_error, out.divergent, out.tree_depth, out.n_leapfrog):
            assert q.shape == (6, 40)
        assert out.run == e.hmc_runs > 0 and out.accept_prob.mean() > 0.5                # chains that move (stuck ones are constant: NaN)
        assert np.all(out.tree_depth >= 1) and np.all(out.tree_depth <= 6) and np.all(out.n_leapfrog >= 1) and np.all(out.n_leapfrog <= 63)
        assert out.step_size.shape == (6,) and np.all(out.step_size > 0) and np.all(out.step_size != 10 ** -0.25)
        assert "chains: 6" in str(out) and "NUTS" in str(out)
        s = out.summary()
        assert s.nchains == 6 and s.ndraws == 40 and s.rhat.shape == (10,) and np.all(np.isfinite(s.rhat)) and np.isfinite(s.lp["ess_bulk"])
        fixed = pfmi_mod.nuts(res, 5, nchains=2, step_size=0.2, max_depth=4)
        assert fixed.draws.shape == (10, 5, 2) and np.all(fixed.step_size == 0.2) and np.all(fixed.tree_depth <= 4)
        with pytest.raises(ValueError, match="max_depth"):
            pfmi_mod.nuts(res, 5, max_depth=11)
    finally:
        e.close()


def test_return_codes(pfmi_mod):
    """every return code of pfmi_nuts_* through the C ABI; the ctx stays usable afterwards"""
    from pfmi import _lib
    L = _lib.lib()
    i64p, u64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    d, K = 12, 2
    tg = pfmi_mod.t_diag(d, seed=3)
    e = pfmi_mod.Engine(0)
    x0 = np.asfortranarray(np.repeat(tg.mean[:, None], K, axis=1))
    seeds = np.array([1, 2], dtype=np.uint64)
    fin = C.c_int32()

    def enq(pts=(0, 0), x=x0, sd=seeds, eps=(0.1, 0.1), md=3, T=2, flags=0, k=K):
        pts = np.array(pts, dtype=np.int64)
        eps = np.array(eps, dtype=np.float64)
        return L.pfmi_nuts_enqueue(e.ctx, k, pts.ctypes.data_as(i64p), None if x is None else x.ctypes.data_as(dp),
                                   None if sd is None else sd.ctypes.data_as(u64p), eps.ctypes.data_as(dp), md, T, flags)

    try:
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        assert enq() == -3 and b"fit_batch" in L.pfmi_last_error()                    # PFMI_ERR_STATE: not fitted
        assert L.pfmi_nuts_wait(e.ctx) == -3 and L.pfmi_nuts_pump(e.ctx, C.byref(fin)) == -3
        assert L.pfmi_nuts_get_stats(e.ctx, None, None) == -3 and L.pfmi_nuts_get_path(e.ctx, 0, 1, None, None, None, None) == -3
        assert L.pfmi_nuts_stats(e.ctx, None, None) == -3 and L.pfmi_nuts_pump(e.ctx, None) == -1
        e.fit_batch(6)
        assert enq(flags=1) == -3                                                       # CONTINUE without a run
        P = e.P
        for bad in (dict(k=0), dict(pts=(0, P)), dict(pts=(-1, 0)), dict(eps=(0.1, 0.0)), dict(eps=(0.1, np.inf)), dict(eps=(np.nan, 0.1)),
                    dict(md=0), dict(md=11), dict(T=0), dict(x=None), dict(sd=None), dict(flags=4)):
            assert enq(**bad) == -1, bad                                                # PFMI_ERR_ARG
        assert enq() == 0
        assert L.pfmi_hmc_get(e.ctx, None, None, None, None, None) in (0, -3)           # rounds to go: refused; finished already: served
        assert L.pfmi_hmc_wait(e.ctx) == -3                                             # the run is not static HMC's
        assert L.pfmi_nuts_wait(e.ctx) == 0 and L.pfmi_nuts_pump(e.ctx, C.byref(fin)) == 0 and fin.value == 1
        r, n = C.c_int64(), C.c_int64()
        assert L.pfmi_nuts_stats(e.ctx, C.byref(r), C.byref(n)) == 0 and 3 <= r.value <= 15 and n.value >= 2 * r.value
        ptr, cnt = C.c_void_p(), C.c_int64()
        assert L.pfmi_hmc_draws_dev(e.ctx, C.byref(ptr), C.byref(cnt)) == 0 and ptr.value and cnt.value == 4
        assert L.pfmi_nuts_get_stats(e.ctx, None, None) == 0
        assert L.pfmi_nuts_get_path(e.ctx, 0, 1, None, None, None, None) == -3          # the run kept no path
        assert enq(flags=2) == 0 and L.pfmi_nuts_wait(e.ctx) == 0
        assert L.pfmi_nuts_get_path(e.ctx, 0, 1, None, None, None, None) == 0 and L.pfmi_nuts_get_path(e.ctx, 0, 1000, None, None, None, None) == -1
        assert L.pfmi_hmc_get_path(e.ctx, 0, 1, None, None, None) == -3                 # ... and it is not static HMC's path
        assert enq(flags=1) == 0 and enq(flags=1, k=1) == -3                            # CONTINUE with another K
        assert enq() == 0 and L.pfmi_nuts_wait(e.ctx) == 0 and enq(flags=1, md=4) == -1  # CONTINUE beyond the chains' checkpoints
        # a new fit forgets the chains
        assert enq() == 0
        e.fit_batch(6)
        assert L.pfmi_nuts_wait(e.ctx) == -3 and enq(flags=1) == -3
        # PFMI_ERR_UNSUPPORTED: built-in targets, device closures without a gradient, a path that does not fit
        e.set_target(demo_device_target(tg))
        assert enq() == -4 and b"gradient" in L.pfmi_last_error()
        e.set_target(tg)
        assert enq() == -4
        e.set_target(demo_device_target(tg, grad=True))
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        assert enq(md=10, T=2000000, flags=2) == -4 and b"GB" in L.pfmi_last_error()
        # PFMI_ERR_NUMERIC: a point whose fit failed; a start point with a non-finite gradient is reported by the wait
        xbad = x0.copy()
        xbad[0, 1] = np.inf
        assert enq(x=xbad) == 0 and L.pfmi_nuts_wait(e.ctx) == -5
        rng = np.random.default_rng(0)
        e.set_traces([np.cumsum(rng.normal(size=(9, d)), 0)], [rng.normal(size=(9, d))])
        e.fit_batch(5, -1e300)
        status = e.fit_status()[0]
        badp = int(np.flatnonzero(status != 0)[0])
        assert enq(pts=(0, badp)) == -5 and b"status" in L.pfmi_last_error()
        e.optimize_batch(np.ones((1, d)), 6, 30)
        e.fit_batch(6)
        got = _run(e, [0, 0], x0, seeds, 0.1, 3, 3)                                      # ... and the ctx still samples
        assert np.all(np.isfinite(got["draws"]))
    finally:
        e.close()
