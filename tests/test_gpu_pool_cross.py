"""Weighted cross moments of the pool on the device (pfmi_pool_cross / Engine.pool_cross) and the importance covariance built on them
(pfmi.importance_covariance, MultiPathfinderResult.covariance / .correlation).

Primitive: pool_build, pool_get + psis, pool_cross; the full matrix is compared with the longdouble restatement of the definition
(tests/pool_cross_reference.py) on the DOWNLOADED pool and weights.  Bound per entry, derived, not tuned:
|gpu - ref| <= (M + 4) 2^-53 A, M = K N_r added terms (one more with a carry) and A = |C_in| + sum |w t_i t_j|
(pool_cross_reference.bound).  The worst observed ratio is recorded through tests/margins.py (config "pool_cross") and printed.  Every
parity case also asserts C == C.T bit for bit.

Shapes: d = 1 (one entry), 10 (under one 16-block), 17 (a block and a row), 63 / 64 / 65 (the tile edge), 130 (several tiles, off-diagonal
tiles with ragged rows and ragged columns), 257 (odd d), 1000 (many tiles, paired loads), 4100 (the 128 x 128 tile on a large grid,
sampled); N_r = 1, 5, 37, 1000 (one column, N_r % 4 != 0, a ragged last chunk, many groups); K = 1, 3.  The 128 x 128 tile is also
forced at d = 130 and 257 (both load widths) and must return the bits of the 64 x 64 tile."""
import numpy as np
import pytest

import margins as mg
from pool_common import LD, U, J, _pool, check_pool_error_codes, ratio_to_bound, run_two_engines
from pool_cross_reference import bound, covariance, pool_cross

pytestmark = pytest.mark.gpu


def _check(tag, got, ref, A, M):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    r = ratio_to_bound(bound, got, ref, A, M)
    print(f"pool_cross {tag}: worst |gpu - ref| / bound = {r:.3g}")
    mg.check("pool_cross", "C", r, bound=1.0, contract=1.0, ctx=tag)


def _symmetric(C):
    """C == C.T bit for bit"""
    np.testing.assert_array_equal(np.ascontiguousarray(C).view(np.uint64), np.ascontiguousarray(C.T).view(np.uint64))


CASES = [("d1", 1, 1), ("d1", 5, 3), ("lr10", 5, 1), ("lr10", 1000, 3), ("d17", 37, 3), ("d63", 37, 3), ("d64", 37, 3), ("lr65", 37, 3),
         ("d130", 37, 3), ("d257", 37, 3), ("d1000", 5, 1), ("d1000", 37, 3)]


@pytest.mark.parametrize("name,N_r,K", CASES, ids=[f"{n}-N{r}-K{k}" for n, r, k in CASES])
def test_pool_cross_matches_the_longdouble_reference(pfmi_mod, eng, name, N_r, K):
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    w = eng.psis(lr)["weights"]
    center = np.random.default_rng(d + N_r).normal(size=d) * 0.7 + P[:, 0, 0]
    for imp in (True, False):
        for c in (None, center):
            got = eng.pool_cross(0, imp, c)
            assert got.shape == (d, d)
            _symmetric(got)
            ref, A = pool_cross(P, w if imp else None, c)
            _check(f"{name} N_r={N_r} K={K} imp={int(imp)} center={'y' if c is not None else 'n'}", got, ref, A, K * N_r)
    np.testing.assert_array_equal(eng.pool_cross(0, False, center), got)       # two calls: the same bits


def test_large_d_sampled(pfmi_mod, eng):
    """d = 4100: 33 x 33 tiles of 128 (561 workgroups), the last tile row 4 rows high; about 2 x 10^5 random entries and the whole last
    tile row against the reference, the symmetry on the full matrix"""
    N_r, K = 5, 1
    P, lr = _pool(pfmi_mod, eng, "d4100", K, N_r)
    d = P.shape[0]
    assert d == 4100
    w = eng.psis(lr)["weights"]
    center = P[:, 1, 0] * 0.5 + 0.1
    rng = np.random.default_rng(41)
    ii = np.concatenate([rng.integers(0, d, size=200000), np.repeat(np.arange(4096, d), d)])
    jj = np.concatenate([rng.integers(0, d, size=200000), np.tile(np.arange(d), d - 4096)])
    for imp in (True, False):
        got = eng.pool_cross(0, imp, center)
        _symmetric(got)
        wl = w.astype(LD) if imp else np.ones(N_r, dtype=LD)
        keep = (w != 0.0) if imp else np.ones(N_r, dtype=bool)
        T = P[:, keep, 0].astype(LD) - center.astype(LD)[:, None]
        terms = (wl[keep][None, :] * T[ii]) * T[jj]
        _check(f"d4100 sampled imp={int(imp)}", got[ii, jj], terms.sum(axis=1), np.abs(terms).sum(axis=1), K * N_r)


@pytest.mark.parametrize("name", ["d130", "d257"])
def test_the_tile_size_does_not_change_the_bits(pfmi_mod, eng, name):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    eng.psis(lr)
    center = P[:, 2, 1] + 0.25
    L = pfmi_mod.lib()
    a = eng.pool_cross(0, True, center)
    assert L.pfmi_debug_set(b"PFMI_POOL_CROSS_TILE", b"128") == 0
    try:
        b = eng.pool_cross(0, True, center)
        bc = eng.pool_cross(0, False, None, carry=a)
    finally:
        assert L.pfmi_debug_set(b"PFMI_POOL_CROSS_TILE", None) == 0
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.pool_cross(0, False, None, carry=a), bc)


@pytest.mark.parametrize("name,N_r", [("lr65", 37), ("d130", 37), ("lr10", 1000), ("d1000", 5)])
def test_carry(pfmi_mod, eng, name, N_r):
    """a random symmetric carry stays within the bound with M + 1 terms; runs {0, 1, 2} in one call == run {0}, then runs {1, 2}
    with the first result as the carry (the engine rebuilt; it keeps the PSIS weights of the K = 3 pool): the same bits"""
    P3, lr3 = _pool(pfmi_mod, eng, name, 3, N_r)
    d = P3.shape[0]
    w = eng.psis(lr3)["weights"]
    center = P3[:, 0, 2] * 0.5 + 0.1
    X = np.random.default_rng(3).normal(size=(d, d)) * 10.0
    X = np.tril(X) + np.tril(X, -1).T
    got = eng.pool_cross(0, True, center, carry=X)
    _symmetric(got)
    ref, A = pool_cross(P3, w, center, X)
    _check(f"{name} carry", got, ref, A, 3 * N_r + 1)
    whole = {imp: eng.pool_cross(0, imp, center) for imp in (True, False)}
    _pool(pfmi_mod, eng, name, 1, N_r, runs=[0])
    first = {imp: eng.pool_cross(0, imp, center) for imp in (True, False)}
    P12, _ = _pool(pfmi_mod, eng, name, 2, N_r, runs=[1, 2])
    np.testing.assert_array_equal(P12, P3[:, :, 1:])              # (precondition: the same draws)
    for imp in (True, False):
        np.testing.assert_array_equal(eng.pool_cross(N_r, imp, center, carry=first[imp]), whole[imp], err_msg=f"imp={imp}")
    assert not np.array_equal(eng.pool_cross(N_r, True, center), whole[True])      # (without the carry: another answer)


def test_col_offset_into_a_longer_psis_vector(pfmi_mod, eng):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "lr65", K, N_r)
    rng = np.random.default_rng(8)
    off = 2 * N_r + 5
    glob = np.concatenate([rng.normal(size=off) + lr.mean(), lr, rng.normal(size=50) + lr.mean()])
    w = eng.psis(glob)["weights"]
    got = eng.pool_cross(off, True, None)
    ref, A = pool_cross(P, w[off:off + K * N_r], None)
    _check("col_offset", got, ref, A, K * N_r)
    assert not np.array_equal(eng.pool_cross(0, True, None), got)   # another window of the weights: another answer


def test_zero_weights_are_skipped(pfmi_mod, eng):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "diag30", K, N_r)
    d = P.shape[0]
    lr = lr.copy()
    lr[N_r + 3:2 * N_r + 9] = -np.inf                            # a block across two runs
    lr[0] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.all(w[N_r + 3:2 * N_r + 9] == 0.0) and w[0] == 0.0 and np.count_nonzero(w) >= N_r
    center = P[:, 1, 1] + 0.25
    for c in (None, center):
        ref, A = pool_cross(P, w, c)
        _check("zero weights", eng.pool_cross(0, True, c), ref, A, K * N_r)
    # a run whose columns all have weight 0 changes nothing: the output is the carry
    _pool(pfmi_mod, eng, "diag30", 1, N_r, runs=[1])
    lr[N_r:2 * N_r] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.all(w[N_r:2 * N_r] == 0.0)
    X = np.random.default_rng(4).normal(size=(d, d))
    X = np.tril(X) + np.tril(X, -1).T
    np.testing.assert_array_equal(eng.pool_cross(N_r, True, center, carry=X), X)
    np.testing.assert_array_equal(eng.pool_cross(N_r, True, center), np.zeros((d, d)))


@pytest.mark.parametrize("name", ["lr10", "lr65", "d130", "d1000"])
def test_nan_under_a_zero_weight_is_invisible_and_under_a_weight_poisons_its_row_and_column(pfmi_mod, eng, name):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    z, c = N_r + 20, 2 * N_r + 36                                  # columns of runs 1 and 2 (the ragged last chunk of run 2)
    r0, r1 = d // 2, d - 1
    lr = lr.copy()
    lr[z] = -np.inf
    w = eng.psis(lr)["weights"]
    assert w[z] == 0.0 and w[c] != 0.0
    center = P[:, 0, 0] * 0.5
    base = eng.pool_cross(0, True, center)
    assert np.all(np.isfinite(base))
    ptr, count = eng.pool_draws_dev()
    assert count == d * K * N_r
    nan = np.array([np.nan])

    eng.memcpy_h2d(ptr + 8 * (z * d + r0), nan)                    # under a zero weight: invisible
    Pn = eng.pool_get()[0]
    assert np.isnan(Pn[r0, z % N_r, z // N_r]) and np.count_nonzero(np.isnan(Pn)) == 1
    np.testing.assert_array_equal(eng.pool_cross(0, True, center), base)
    uni = eng.pool_cross(0, False, center)                         # unit weights skip nothing: row and column r0
    bad = np.zeros((d, d), dtype=bool)
    bad[r0, :] = bad[:, r0] = True
    np.testing.assert_array_equal(np.isnan(uni), bad)

    eng.memcpy_h2d(ptr + 8 * (c * d + r1), nan)                    # under a non-zero weight: exactly row r1 and column r1
    got = eng.pool_cross(0, True, center)
    bad = np.zeros((d, d), dtype=bool)
    bad[r1, :] = bad[:, r1] = True
    np.testing.assert_array_equal(np.isnan(got), bad)
    np.testing.assert_array_equal(got[~bad], base[~bad])           # every other entry has the bits of the clean run


def test_error_codes(pfmi_mod):
    def then(e):
        assert e.L.pfmi_pool_cross(e.ctx, 0, 0, None, None, None) == -1       # c_out NULL
        with pytest.raises(ValueError):
            e.pool_cross(0, False, np.zeros(3))
        for bad in (np.zeros((10, 9)), np.zeros(100)):
            with pytest.raises(ValueError):
                e.pool_cross(0, False, None, carry=bad)

    check_pool_error_codes(pfmi_mod, lambda e, off, imp: e.pool_cross(off, imp), then)


@pytest.mark.parametrize("d,r", [(10, 3), (65, 8)])
def test_importance_covariance_of_a_multipathfinder_result(pfmi_mod, d, r):
    """cov against the reference's two-pass covariance of the pool downloaded after the call.  Tolerance, with M = K N_r, n = M + 5 and
    A the absolute sums of the cross moments about the mean: C is within (M + 4) u A of its exact value and W = sum w carries
    (N_r + K + 3) u relative, so C / W is within 2 n u A / W (one u for the division); cov = C / W - delta delta' does not depend on
    the centre, delta delta' is of the order of u^2 and the subtraction rounds once more: 2 (n + 1) u A / W.  summary().var is within
    2 (N_r + K + 6) u A_ii / W of the same variance (test_gpu_pool_moments._summary_bounds), so diag(cov) and var differ by at most
    the sum of the two.  np.cov(pool, ddof=0) is itself a float64 dot of M terms about a rounded mean: the same form again, so the
    uniform covariance is within 4 (n + 1) u A / W of it."""
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        tg = pfmi.t_lowrank(d, r=r, seed=2)
        res = pfmi.multipathfinder(tg, 100, nruns=3, ndraws_per_run=50, rng=pfmi.HostRNG(4), engine=e)
        K, N_r = 3, 50
        c = res.covariance()
        assert isinstance(c, pfmi.ImportanceCovariance) and c.pareto_shape == res.psis_result.pareto_shape
        assert c.cov.shape == (d, d) and c.corr.shape == (d, d) and c.mean.shape == (d,) and c.ncandidates == K * N_r
        P = np.array(e.pool_get()[0])                            # the pool the call rebuilt
        np.testing.assert_array_equal(P, np.stack([x.draws for x in res.pathfinder_results], axis=2))
        w = res.psis_result.weights
        n = K * N_r + 5
        s = res.summary()
        for tag, got, ww in (("weighted", c, w), ("uniform", res.covariance(importance=False), None)):
            ref = covariance(P, ww)
            tol = 2 * (n + 1) * U * ref["A"] / ref["W"]
            ratio = float(np.max(np.abs(got.cov.astype(LD) - ref["cov"]) / tol))
            print(f"importance_covariance d={d} {tag}: worst |cov - ref| / tolerance = {ratio:.3g}")
            mg.check("pool_cross", "cov", ratio, bound=1.0, contract=1.0, ctx=f"d={d} {tag}")
            _symmetric(got.cov)
            _symmetric(got.corr)
            np.testing.assert_array_equal(np.diagonal(got.corr), np.ones(d))
            assert np.all(np.abs(got.corr) <= 1 + 1e-12)
        np.testing.assert_array_equal(c.mean, s.mean)
        assert c.ess == s.ess
        ref = covariance(P, w)
        tol_d = 2 * (n + 1 + N_r + K + 6) * U * np.diagonal(ref["A"]) / ref["W"]
        rd = float(np.max(np.abs(np.diagonal(c.cov).astype(LD) - s.var.astype(LD)) / tol_d))
        print(f"importance_covariance d={d}: worst |diag(cov) - summary().var| / tolerance = {rd:.3g}")
        mg.check("pool_cross", "diag_vs_var", rd, bound=1.0, contract=1.0, ctx=f"d={d}")
        u = res.covariance(importance=False)
        assert np.isnan(u.pareto_shape) and u.ess == float(K * N_r)
        refu = covariance(P, None)
        tol_u = 4 * (n + 1) * U * refu["A"] / refu["W"]
        ru = float(np.max(np.abs(u.cov.astype(LD) - np.cov(P.reshape(d, -1, order="F"), ddof=0).astype(LD)) / tol_u))
        print(f"importance_covariance d={d}: worst |uniform cov - np.cov| / tolerance = {ru:.3g}")
        mg.check("pool_cross", "cov_vs_numpy", ru, bound=1.0, contract=1.0, ctx=f"d={d}")
        np.testing.assert_array_equal(res.correlation(), c.corr)
        np.testing.assert_array_equal(pfmi.importance_covariance(res).cov, c.cov)
        e.fit_batch(J)                                           # the engine is refitted: the stored handles are stale
        with pytest.raises(pfmi.StaleHandleError):
            res.covariance()
    finally:
        e.close()


_MULTI = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/pathfinder.jl_amd")
import pfmi
tg = pfmi.t_lowrank(65, r=8, seed=2)
one = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4))
engs = [pfmi.Engine(0), pfmi.Engine(0)]
two = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4), engines=engs)
assert len({id(r.fit_distribution.engine) for r in two.pathfinder_results}) == 2
for imp in (True, False):
    a, b = (pfmi.importance_covariance(r, importance=imp) for r in (one, two))
    assert np.array_equal(a.cov, b.cov) and np.array_equal(a.corr, b.corr) and np.array_equal(a.mean, b.mean) and a.ess == b.ess, imp
    assert np.array_equal(a.cov, a.cov.T) and np.all(np.isfinite(a.cov))
    # the primitive over the two engines, chained through the carry, has the bits of the one engine
    off = len(two.pathfinder_results) // 2 * 50
    c0 = one.engine.pool_cross(0, imp, a.mean)
    c1 = engs[0].pool_cross(0, imp, a.mean)
    c2 = engs[1].pool_cross(off, imp, a.mean, carry=c1)
    assert np.array_equal(c2, c0) and not np.array_equal(c1, c0)
print("covariance engines ok")
"""


@pytest.mark.timeout(600)
def test_covariance_over_two_engines_is_bit_identical():
    """engines=[Engine(0), Engine(0)] through the RCCL stand-in: the covariance and the chained primitive have the bits of the
    one-engine result"""
    run_two_engines(_MULTI, "covariance engines ok")
