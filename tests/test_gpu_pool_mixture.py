"""Mixture-proposal weights of the pooled draws (pfmi_pool_mixture_ratios, csrc/pool_mixture_kernels.hip): the bits of the existing
component kernels at d <= 1024, the row-tiled kernel against a long-double reference at every shape where it takes another path,
invariance under chunking / group size / pool position, the identities that tie the mixture weights to the per-run ones, special
values, error codes, and the public `proposal="mixture"` route.

The bound of the tiled kernel is not a fixed number: on the same columns the lane route (pfmi_mixture_logpdf at d > 1024, not code
under test) is measured against the same reference, and the tiled kernel may be at most 4 x as far off relative to max(|lse|, 1), with
the floor 1e-13 that test_gpu_mixture_geometry.py asserts (pool_mixture_common.tiled_bound)."""
import ctypes as C

import numpy as np
import pytest

import margins as mg
import mixture_reference as R
import pool_mixture_common as M
from helpers import make_traces
from pool_common import J as POOL_J, _pool, _traces

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.SKIP_REASON)
_i64p = C.POINTER(C.c_int64)


def _bits(a, b, what=None):
    np.testing.assert_array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64),
                                  err_msg=str(what))


def _hook(pfmi_mod, name, val):
    assert pfmi_mod.lib().pfmi_debug_set(name.encode(), str(val).encode() if val else None) == 0


def _ratios(pfmi_mod, eng, chunk=None, cpb=None):
    """(log_mix, log_ratios) with the chunk length / group size forced for this call only"""
    _hook(pfmi_mod, "PFMI_POOL_MIX_CHUNK", chunk)
    _hook(pfmi_mod, "PFMI_MIXTURE_CPB", cpb)
    try:
        return eng.pool_mixture_ratios()
    finally:
        _hook(pfmi_mod, "PFMI_POOL_MIX_CHUNK", None)
        _hook(pfmi_mod, "PFMI_MIXTURE_CPB", None)


def _cols(P, d):
    return np.asfortranarray(P).reshape(d, -1, order="F")


def _pool_lp(eng, pts, seeds, N_r, lr):
    """(logp, logq) of the pool's columns with the pool's bits: the draws of (fit, seed) regenerated; checked against the pool's ratios"""
    blocks = [eng.draws(p, int(s), N_r) for p, s in zip(pts, seeds)]
    lp, lq = np.concatenate([b[1] for b in blocks]), np.concatenate([b[2] for b in blocks])
    _bits(lp - lq, lr, "pool_lp - pool_lq is not the pool's log ratio")
    return lp, lq


def _named_pool(pfmi_mod, eng, name, K, N_r, runs=None):
    """a pool of pool_common's named case: (pts, seeds, X (d, K N_r), lr)"""
    P, lr = _pool(pfmi_mod, eng, name, K, N_r, runs=runs)
    runs = list(runs) if runs is not None else list(range(K))
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(len(runs))]
    return pts, [1000 + 7 * r for r in runs], _cols(P, eng.d), lr


_GRID_TRACES = {}


def _grid_pool(pfmi_mod, eng, J, d, N_r, runs):
    """a pool of the (J, d) row of mixture_reference's grid: run r < 2 is path r with its first fit of full history, run 2 is path 0
    again with a later fit (the grid has two paths); seeds as in pool_common.  (pts, seeds, X, lr)"""
    if (J, d) not in _GRID_TRACES:
        _GRID_TRACES[(J, d)] = R.grid_traces(pfmi_mod, J, d)
    trs = [_GRID_TRACES[(J, d)][r % 2] for r in runs]
    eng.set_target(R.grid_target(pfmi_mod, d))
    eng.set_traces([t.points for t in trs], [t.gradients for t in trs])
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    pts = []
    for k, r in enumerate(runs):
        p0, p1 = int(eng.offsets[k]), int(eng.offsets[k + 1])
        cand = p0 + np.flatnonzero((jeff[p0:p1] == J) & (status[p0:p1] == 0))
        assert len(cand) >= 8, (J, d, r, len(cand))
        pts.append(int(cand[0] if r < 2 else cand[len(cand) // 4]))
    seeds = [1000 + 7 * r for r in runs]
    eng.pool_build(N_r, pts, np.array(seeds, dtype=np.uint64))
    P, lr = eng.pool_get()
    X = _cols(P, d)
    assert np.all(np.isfinite(X))
    return pts, seeds, X, lr


def _shape_pool(pfmi_mod, eng, J, d, N_r, K, runs=None):
    runs = list(runs) if runs is not None else list(range(K))
    if d == 10000:
        assert J == POOL_J
        return _named_pool(pfmi_mod, eng, "d10000", len(runs), N_r, runs=runs)
    return _grid_pool(pfmi_mod, eng, J, d, N_r, runs)


_BOUNDS = {}


def _tiled_case(pfmi_mod, eng, J, d, N_r, K):
    """build the pool, run the call, measure the tiled kernel and the lane route against the long-double reference; the case's numbers
    are kept for the identities"""
    key = (J, d, N_r, K)
    pts, seeds, X, lr = _shape_pool(pfmi_mod, eng, J, d, N_r, K)
    lm, lrm = eng.pool_mixture_ratios()
    lane = eng.mixture_logpdf(pts, X) - M.log_k(K)
    if key not in _BOUNDS:
        jeff = eng.fit_status()[1]
        ref = M.lse_ld(np.stack([R.ref_logpdf(eng.get_fit(p, int(jeff[p])), X) for p in pts])) - np.log(M.LD(K))
        lane_err, tiled_err = M.rel_to_lse(lane, ref), M.rel_to_lse(lm, ref)
        _BOUNDS[key] = dict(lane=lane_err, tiled=tiled_err, bound=M.tiled_bound(lane_err))
    return dict(pts=pts, seeds=seeds, X=X, lr=lr, lm=lm, lrm=lrm, **_BOUNDS[key])


# ---- 1. the bits of the existing kernels at d <= 1024 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N_r,K", [("lr10", 5, 1), ("funnel12", 37, 3), ("lr65", 37, 3), ("d257", 37, 3), ("d1000", 5, 1)])
def test_bits_of_the_component_kernels_at_small_d(pfmi_mod, eng, name, N_r, K):
    pts, seeds, X, lr = _named_pool(pfmi_mod, eng, name, K, N_r)
    S = K * N_r
    lm, lrm = eng.pool_mixture_ratios()
    ptr, cnt = eng.pool_draws_dev()
    assert cnt == eng.d * S
    buf = eng.malloc_dev(8 * S)
    try:
        p64 = np.ascontiguousarray(pts, dtype=np.int64)
        assert pfmi_mod.lib().pfmi_mixture_logpdf_dev(eng.ctx, C.c_int32(K), p64.ctypes.data_as(_i64p), C.c_int64(S), C.c_void_p(ptr),
                                                      C.c_void_p(buf), None) == 0
        eng.sync()
        lse = eng.memcpy_d2h(np.empty(S), buf)
    finally:
        eng.free_dev(buf)
    _bits(lm, lse - M.log_k(K), name)
    lp, _ = _pool_lp(eng, pts, seeds, N_r, lr)
    _bits(lrm, lp - lm, name)
    _bits(eng.pool_get(draws=False)[1], lr, "pool_get's ratios changed")
    dptr, dcnt = eng.pool_mixture_ratios_dev()
    assert dcnt == S
    _bits(eng.memcpy_d2h(np.empty(S), dptr), lrm, "device pointer")


# ---- 2. the tiled kernel against extended precision ----------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("N_r,K", M.POOLS, ids=lambda v: str(v))
@pytest.mark.parametrize("J,d", M.SHAPES, ids=lambda v: str(v))
def test_tiled_kernel_against_long_double(pfmi_mod, eng, J, d, N_r, K):
    c = _tiled_case(pfmi_mod, eng, J, d, N_r, K)
    cfg = f"pool-mix-J{J}-d{d}-N{N_r}-K{K}"
    print(f"{cfg}: lane route {c['lane']:.3e}  tiled {c['tiled']:.3e}  bound {c['bound']:.3e}")
    assert np.all(np.isfinite(c["lm"])) and np.all(np.isfinite(c["lrm"]))
    mg.check(cfg, "lse@lane_vs_longdouble", c["lane"], bound=1e-9, why="the lane route, measured to set the tiled kernel's bound")
    mg.check(cfg, "lse@tiled_vs_longdouble", c["tiled"], bound=c["bound"], why="4 x the lane route's error, floor 1e-13")
    lp, _ = _pool_lp(eng, c["pts"], c["seeds"], N_r, c["lr"])
    _bits(c["lrm"], lp - c["lm"], cfg)
    _bits(eng.pool_get(draws=False)[1], c["lr"], "pool_get's ratios changed")


# ---- 3. geometry invariance, bit-exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d1000", "J6-d2049"])
def test_chunking_and_group_size_do_not_change_a_bit(pfmi_mod, eng, case):
    if case == "d1000":
        _named_pool(pfmi_mod, eng, "d1000", 3, 37)
    else:
        _grid_pool(pfmi_mod, eng, 6, 2049, 37, [0, 1, 2])
    base = _ratios(pfmi_mod, eng)
    assert np.all(np.isfinite(base[0]))
    for chunk in (16, 17, 1000):
        got = _ratios(pfmi_mod, eng, chunk=chunk)
        _bits(got[0], base[0], (case, chunk))
        _bits(got[1], base[1], (case, chunk))
    for cpb in (1, 2, 3):
        got = _ratios(pfmi_mod, eng, chunk=17, cpb=cpb)
        _bits(got[0], base[0], (case, "cpb", cpb))


@pytest.mark.parametrize("case", ["d1000", "d10000"])
def test_a_run_alone_or_in_the_middle_of_three(pfmi_mod, eng, case):
    """Run 1 pooled alone (K = 1: log_mix IS its own component's logpdf, columns 0 .. 36) and as the middle of three (columns 37 .. 73,
    K = 3).  Only the other components' terms differ: on every column where they lie more than 800 below the run's own (exp underflows to
    an exact zero, so lse is the own component exactly) the K = 3 value must be fl(own - log 3) bit for bit.  The cases are the ones
    whose three fits lie that far apart (three L-BFGS steps from three starting points): d = 1000 for the component kernels of
    mixture_kernels.hip, d = 10 000 for the row-tiled kernel (the fits of the (6, 2049) grid row overlap in every column)."""
    N_r = 37

    def build(runs):
        return _named_pool(pfmi_mod, eng, case, len(runs), N_r, runs=runs)

    pts1, _, X1, _ = build([1])
    own = _ratios(pfmi_mod, eng)[0]
    pts3, _, X3, _ = build([0, 1, 2])
    _bits(X3[:, N_r:2 * N_r], X1, "the run's columns")
    lm3 = _ratios(pfmi_mod, eng)[0][N_r:2 * N_r]
    _, comp = eng.mixture_logpdf(pts3, X1, componentwise=True)
    alone = np.all(comp[:, [0, 2]] < comp[:, [1]] - 800, axis=1)
    print(f"{case}: {int(alone.sum())} of {N_r} columns see only their own component")
    assert alone.any(), comp[:3]
    _bits(lm3[alone], (own - M.log_k(3))[alone], case)
    others = ~alone                                      # elsewhere the other components can only add mass
    assert np.all(lm3[others] >= (own - M.log_k(3))[others] - 1e-13 * np.maximum(np.abs(own[others]), 1))


@pytest.mark.parametrize("case", ["d1000", "J6-d2049"])
def test_a_column_has_the_same_bits_at_5_and_37_draws_per_run(pfmi_mod, eng, case):
    build = ((lambda n: _named_pool(pfmi_mod, eng, "d1000", 1, n)) if case == "d1000"
             else (lambda n: _grid_pool(pfmi_mod, eng, 6, 2049, n, [0])))
    _, _, X5, _ = build(5)
    lm5, lr5 = _ratios(pfmi_mod, eng)
    _, _, X37, _ = build(37)
    lm37, lr37 = _ratios(pfmi_mod, eng)
    _bits(X37[:, :5], X5)
    _bits(lm37[:5], lm5, case)
    _bits(lr37[:5], lr5, case)


# ---- 4. identities ----------------------------------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("J,d", M.SHAPES, ids=lambda v: str(v))
def test_one_component_gives_the_per_run_ratios(pfmi_mod, eng, J, d):
    """K = 1: the mixture is the run's own fit, so the mixture ratio is the per-run ratio up to the rounding of two different kernels
    (the scan forms logq from the normals, the mixture kernel from the draw)"""
    c = _tiled_case(pfmi_mod, eng, J, d, 1, 1)
    _, lq = _pool_lp(eng, c["pts"], c["seeds"], 1, c["lr"])
    dev = np.abs(c["lrm"] - c["lr"]) / np.maximum(np.abs(lq), 1)
    print(f"K=1 J={J} d={d}: |mixture ratio - per-run ratio| / max(|logq|, 1) = {float(dev.max()):.3e}, bound {c['bound']:.3e}")
    mg.check(f"pool-mix-J{J}-d{d}-N1-K1", "logratio@mixture_vs_scan", dev, bound=c["bound"],
             why="the bound of the tiled kernel against long double")


@pytest.mark.parametrize("case", ["lr10", "J6-d2049"])
def test_the_same_fit_twice_is_the_fit(pfmi_mod, eng, case):
    """K = 2 with one fit and one seed twice: lse = v + log 2, minus log 2: the K = 1 value to 2 ulp of max(|v|, 1)"""
    if case == "lr10":
        _named_pool(pfmi_mod, eng, "lr10", 1, 5, runs=[1])
        one = eng.pool_mixture_ratios()[0]
        _, _, X2, _ = _named_pool(pfmi_mod, eng, "lr10", 2, 5, runs=[1, 1])
    else:
        _grid_pool(pfmi_mod, eng, 6, 2049, 5, [0])
        one = eng.pool_mixture_ratios()[0]
        _, _, X2, _ = _grid_pool(pfmi_mod, eng, 6, 2049, 5, [0, 0])
    _bits(X2[:, :5], X2[:, 5:], "the two runs' columns")
    two = eng.pool_mixture_ratios()[0]
    for blk in (two[:5], two[5:]):
        assert np.all(np.abs(blk - one) <= 2 * np.spacing(np.maximum(np.abs(one), 1))), (blk, one)


@needs_ld
@pytest.mark.parametrize("N_r,K", M.POOLS, ids=lambda v: str(v))
@pytest.mark.parametrize("J,d", M.SHAPES, ids=lambda v: str(v))
def test_the_mixture_is_at_least_the_own_component_over_K(pfmi_mod, eng, J, d, N_r, K):
    """qbar >= q_own / K, so log_mix >= logq_own - log K, with logq_own = pool_lp - pool_lr recovered on the host"""
    c = _tiled_case(pfmi_mod, eng, J, d, N_r, K)
    lp, _ = _pool_lp(eng, c["pts"], c["seeds"], N_r, c["lr"])
    own = lp - c["lr"]
    slack = c["bound"] * np.maximum(np.abs(own), 1)
    short = (own - M.log_k(K)) - c["lm"]
    print(f"J={J} d={d} N_r={N_r} K={K}: largest shortfall / slack {float(np.max(short / slack)):.3f}")
    assert np.all(short <= slack), float(np.max(short / slack))


# ---- 5. special values ------------------------------------------------------------------------------------------------------------------------
def test_a_failed_component_makes_every_column_nan(pfmi_mod, eng):
    """the failed-fit construction of mixture_reference.FAILED; pool_build accepts a failed fit's point (its draws are NaN rows of the
    log densities), and the mixture of the pool is NaN everywhere: one of its components has no density"""
    Jf, d = R.FAILED
    rng = np.random.default_rng(0)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(9, d)), 0), rng.normal(size=(9, d))
    tg = pfmi_mod.t_diag(d, seed=3)
    good = make_traces(tg, 1, 3)[0]
    eng.set_target(tg)
    eng.set_traces([bad_th, good.points], [bad_gr, good.gradients])
    eng.fit_batch(Jf, -1e300)
    status, jeff, _, _ = eng.fit_status()
    bad = [p for p in range(9) if status[p] != 0]
    assert bad, status
    ok = 9 + len(good) - 1
    assert status[ok] == 0
    eng.pool_build(5, [bad[0], ok], np.array([1, 2], dtype=np.uint64))
    lm, lrm = eng.pool_mixture_ratios()
    assert np.all(np.isnan(lm)) and np.all(np.isnan(lrm)), (lm, lrm)


def test_target_nan_and_minus_infinity_propagate(pfmi_mod, eng):
    """logp values prescribed through a host closure: NaN where the first coordinate is large, -inf where the second is"""
    tg, traces = _traces(pfmi_mod, "lr10")
    thr = 0.3

    def logp_batch(X):
        v = np.asarray(tg.logp(X), dtype=np.float64).copy()
        v[X[1] > tg.mean[1] + thr] = -np.inf
        v[X[0] > tg.mean[0] + thr] = np.nan
        return v

    cb = pfmi_mod.CallbackTarget(10, lambda x: float(logp_batch(np.asarray(x)[:, None])[0]), grad=tg.grad, logp_batch=logp_batch)
    eng.set_target(cb)
    eng.set_traces([t.points for t in traces[:2]], [t.gradients for t in traces[:2]])
    eng.fit_batch(POOL_J)
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(2)]
    eng.pool_build(37, pts, np.array([1000, 1007], dtype=np.uint64))
    P, lr = eng.pool_get()
    X = _cols(P, 10)
    nan = X[0] > tg.mean[0] + thr
    ninf = (X[1] > tg.mean[1] + thr) & ~nan
    assert nan.any() and ninf.any() and (~nan & ~ninf).any()
    lm, lrm = eng.pool_mixture_ratios()
    assert np.all(np.isfinite(lm))
    assert np.all(np.isnan(lrm[nan])) and np.all(lrm[ninf] == -np.inf) and np.all(np.isfinite(lrm[~nan & ~ninf]))
    assert np.all(np.isnan(lr[nan])) and np.all(lr[ninf] == -np.inf)             # (the per-run ratios follow the same rule)


@pytest.mark.parametrize("case", ["lr10", "J6-d1057"])
def test_a_column_50_standard_deviations_out_is_not_nan(pfmi_mod, eng, case):
    """a finite column far in the tail of every component, written into the pool behind pfmi_pool_draws_dev: small, never NaN"""
    if case == "lr10":
        pts, _, X, _ = _named_pool(pfmi_mod, eng, "lr10", 2, 5)
    else:
        pts, _, X, _ = _grid_pool(pfmi_mod, eng, 6, 1057, 5, [0, 1])
    d = eng.d
    before = eng.pool_mixture_ratios()[0]
    f = eng.get_fit(pts[0], int(eng.fit_status()[1][pts[0]]))
    lam, v = R._top_eig(f)
    far = np.ascontiguousarray(f["mu"] + 50 * np.sqrt(lam) * v)
    assert np.all(np.isfinite(far))
    ptr, _ = eng.pool_draws_dev()
    g = 3
    eng.memcpy_h2d(ptr + 8 * d * g, far)
    lm, lrm = eng.pool_mixture_ratios()
    assert not np.isnan(lm[g]) and not np.isnan(lrm[g]), (lm[g], lrm[g])
    assert lm[g] < before[g]
    keep = np.arange(len(lm)) != g
    _bits(lm[keep], before[keep], "the other columns")


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(pfmi_mod):
    e = pfmi_mod.Engine(0)
    try:
        tg, traces = _traces(pfmi_mod, "lr10")
        e.set_target(tg)
        e.set_traces([t.points for t in traces[:2]], [t.gradients for t in traces[:2]])
        e.fit_batch(POOL_J)
        for call in (e.pool_mixture_ratios, e.pool_mixture_ratios_dev):               # no pool
            with pytest.raises(pfmi_mod.PfmiError) as ex:
                call()
            assert ex.value.code == -3
        pts = [int(e.offsets[k + 1]) - 1 for k in range(2)]
        e.pool_build(5, pts, np.array([1, 2], dtype=np.uint64))
        with pytest.raises(pfmi_mod.PfmiError) as ex:                                   # _dev before the host call
            e.pool_mixture_ratios_dev()
        assert ex.value.code == -3
        e.pool_mixture_ratios()
        assert e.pool_mixture_ratios_dev()[1] == 10
        e.pool_build(5, pts, np.array([1, 2], dtype=np.uint64))
        with pytest.raises(pfmi_mod.PfmiError) as ex:                                   # a new pool invalidates the result
            e.pool_mixture_ratios_dev()
        assert ex.value.code == -3
    finally:
        e.close()


# ---- 7. the public route ------------------------------------------------------------------------------------------------------------------------
def test_public_route(pfmi_mod, eng):
    tg = pfmi_mod.t_lowrank(10, r=3, seed=3)
    kw = dict(nruns=4, ndraws_elbo=50, engine=eng)
    res = pfmi_mod.multipathfinder(tg, 100, rng=pfmi_mod.HostRNG(5), proposal="mixture", **kw)
    assert res.proposal == "mixture" and res.ndraws_per_run == 50
    runs = res.pathfinder_results
    # the same weights through the public pieces: the runs' stored draws and target values, the mixture's logpdf, PSIS
    blocks = [eng.draws(r.fit_distribution.point, r.draw_seed, 50) for r in runs]
    pool = np.asfortranarray(np.concatenate([b[0] for b in blocks], axis=1))
    lp = np.concatenate([b[1] for b in blocks])
    psis = eng.psis(lp - res.fit_distribution.logpdf(pool))
    dev = np.max(np.abs(psis["log_weights"] - res.psis_result.log_weights)) / (1 + np.abs(psis["log_weights"]).max())
    # the same kernels on the same bits, up to the last bit of log 4 (NumPy's here, the C library's in the call): far inside the contract
    mg.check("pool-mix-public", "psis_logw", dev, bound=1e-12)
    mg.check("pool-mix-public", "pareto_k", abs(psis["pareto_shape"] - res.psis_result.pareto_shape))
    idx = eng.resample_indices(200, 100, seed=int(pfmi_mod.HostRNG(5).rand_u64(5)[4]))
    np.testing.assert_array_equal(res.draw_component_ids, idx // 50 + 1)
    _bits(res.draws, pool[:, idx])
    summ = res.summary()
    assert summ.pareto_shape == res.psis_result.pareto_shape
    again = pfmi_mod.resample(res, 100)
    assert again.proposal == "mixture"
    _bits(again.psis_result.log_weights, res.psis_result.log_weights)
    fresh = pfmi_mod.resample(res, 100, ndraws_per_run=60)
    assert fresh.proposal == "mixture" and len(fresh.psis_result.weights) == 240 and fresh.draws.shape == (10, 100)
    plain = pfmi_mod.resample(res, 100, proposal="component")
    assert plain.proposal == "component" and plain.psis_result is not res.psis_result
    # "component" and no keyword: identical bits
    a = pfmi_mod.multipathfinder(tg, 100, rng=pfmi_mod.HostRNG(5), proposal="component", **kw)
    mean_a = a.summary().mean
    b = pfmi_mod.multipathfinder(tg, 100, rng=pfmi_mod.HostRNG(5), **kw)
    assert a.proposal == b.proposal == "component"
    _bits(a.draws, b.draws)
    _bits(a.psis_result.weights, b.psis_result.weights)
    _bits(mean_a, b.summary().mean)
    print(f"k-hat on lowrank d=10, K=4: component {a.psis_result.pareto_shape:.3f}  mixture {res.psis_result.pareto_shape:.3f}")
    mg.record("pool-mix-public", "khat@component", a.psis_result.pareto_shape, np.inf)
    mg.record("pool-mix-public", "khat@mixture", res.psis_result.pareto_shape, np.inf)
    e2 = pfmi_mod.Engine(0)
    try:
        with pytest.raises(ValueError, match="one engine"):
            pfmi_mod.multipathfinder(tg, 100, nruns=4, ndraws_elbo=50, engines=[eng, e2], proposal="mixture")
    finally:
        e2.close()
