"""The pooled second moment applied to a thin block of vectors on the device (pfmi_pool_apply / Engine.pool_apply) and the low-rank
covariance built on it (pfmi.importance_lowrank_covariance, MultiPathfinderResult.lowrank_covariance).

Primitive: pool_build, pool_get + psis, pool_apply; scores and Y are compared with the longdouble restatement of the two definitions
(tests/pool_apply_reference.py) on the DOWNLOADED pool and weights.  Bounds per entry, derived, not tuned:
  scores  |gpu - ref| <= (d + 4) 2^-53 A_z, A_z = sum_i |t_i v_ji|                               (pool_apply_reference.bound_scores)
  Y       against the reference evaluated with the downloaded DEVICE scores as the second operand:
          |gpu - ref| <= (M + 4) 2^-53 A_Y, M = K N_r added terms (one more with a carry), A_Y = |y_in| + sum |w t_i z_j|   (.bound)
  Y       once per case against the all-longdouble C V: the A_Y term plus what the scores' own error adds,
          sum_n |w t_i| (d + 4) u A_z(n)                                                           (.propagated)
The worst observed ratios are recorded through tests/margins.py (config "pool_apply") and printed.

Shapes: d = 1, 3 (under one group of 4 rows), 10, 17, 63 / 64 / 65 (the tile edge), 130, 257 (odd d, several tiles), 1000 (paired loads),
10 000 (scores in full, Y on sampled rows); N_r = 1, 5, 37, 1000 (one column, N_r % 4 != 0, a ragged last chunk, many chunks); K = 1, 3;
r = 1, 5, 16, 17, 32 (one block, a full block, a block and a direction, two full blocks)."""
import numpy as np
import pytest

import margins as mg
from pool_apply_reference import bound, bound_scores, pool_apply, pool_scores, propagated
from pool_common import LD, U, J, _pool, check_pool_error_codes, ratio_to_bound, run_two_engines
from pool_cross_reference import covariance

pytestmark = pytest.mark.gpu


def _check(quantity, tag, got, ref, b):
    """record and assert max |got - ref| / b <= 1 (an entry with b = 0 must be exact)"""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    r = ratio_to_bound(lambda n, A: A, got, ref, b, 0)
    print(f"pool_apply {quantity} {tag}: worst |gpu - ref| / bound = {r:.3g}")
    mg.check("pool_apply", quantity, r, bound=1.0, contract=1.0, ctx=tag)


def _bits(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64), err_msg=msg)


def _dirs(seed, r, d):
    return np.random.default_rng(seed).normal(size=(r, d))


def _parity(tag, eng, P, w, center, V, rows=None, full=True):
    """one call against the reference: the scores, Y given the device scores and (full) Y against the all-longdouble product"""
    d, N_r, K = P.shape
    Y, Z = eng.pool_apply(0, w is not None, center, V, want_scores=True)
    assert Y.shape == V.shape and Z.shape == (K * N_r, V.shape[0])
    Zr, Az = pool_scores(P, w, center, V)
    _check("scores", tag, Z, Zr, bound_scores(d, Az))
    Yg = Y if rows is None else Y[:, rows]
    Yr, Ay = pool_apply(P, w, center, Z, rows=rows)
    _check("Y", tag, Yg, Yr, bound(K * N_r, Ay))
    if full:
        Yl, Al = pool_apply(P, w, center, Zr, rows=rows)
        _check("Y_exact", tag, Yg, Yl, bound(K * N_r, Al) + propagated(P, w, center, Az, rows=rows))
    return Y, Z


CASES = [("d1", 1, 1, 1), ("d1", 5, 3, 5), ("d3", 5, 3, 5), ("lr10", 5, 1, 5), ("lr10", 1000, 3, 16), ("d17", 37, 3, 17), ("d63", 37, 3, 32),
         ("d64", 37, 3, 16), ("lr65", 37, 3, 5), ("lr65", 1, 3, 1), ("d130", 37, 3, 17), ("d130", 1000, 1, 5), ("d257", 37, 3, 32),
         ("d1000", 5, 1, 16), ("d1000", 37, 3, 5)]


@pytest.mark.parametrize("name,N_r,K,r", CASES, ids=[f"{n}-N{nr}-K{k}-r{r}" for n, nr, k, r in CASES])
def test_pool_apply_matches_the_longdouble_reference(pfmi_mod, eng, name, N_r, K, r):
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    w = eng.psis(lr)["weights"]
    center = np.random.default_rng(d + N_r).normal(size=d) * 0.7 + P[:, 0, 0]
    V = _dirs(d + r, r, d)
    for imp in (True, False):
        for c in (None, center):
            tag = f"{name} N_r={N_r} K={K} r={r} imp={int(imp)} center={'y' if c is not None else 'n'}"
            Y, Z = _parity(tag, eng, P, w if imp else None, c, V, full=c is center)
    Y2, Z2 = eng.pool_apply(0, False, center, V, want_scores=True)             # two calls: the same bits
    _bits(Y2, Y)
    _bits(Z2, Z)
    _bits(eng.pool_apply(0, False, center, V), Y)                              # (and without the download of the scores)


def test_large_d(pfmi_mod, eng):
    """d = 10 000 (157 row tiles, 157 row chunks per score): the scores in full, Y on 400 random rows and the whole last tile"""
    N_r, K, r = 5, 1, 16
    P, lr = _pool(pfmi_mod, eng, "d10000", K, N_r)
    d = P.shape[0]
    assert d == 10000
    w = eng.psis(lr)["weights"]
    center = P[:, 1, 0] * 0.5 + 0.1
    V = _dirs(7, r, d)
    rows = np.concatenate([np.random.default_rng(41).integers(0, d, size=400), np.arange(9984, d)])
    for imp in (True, False):
        for c in (None, center):
            _parity(f"d10000 imp={int(imp)} center={'y' if c is not None else 'n'}", eng, P, w if imp else None, c, V, rows=rows,
                    full=c is center)


@pytest.mark.parametrize("name", ["lr65", "d1000"])
def test_a_direction_does_not_depend_on_the_block(pfmi_mod, eng, name):
    """the r = 32 result restricted to 5 of its directions == the r = 5 call on those directions, and direction 3 of it == the
    r = 1 call given that one vector, bit for bit; with a carry too"""
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    eng.psis(lr)
    center = P[:, 2, 1] + 0.25
    V = _dirs(32, 32, d)
    X = _dirs(33, 32, d) * 5.0
    idx = np.array([3, 0, 17, 31, 16])
    for imp in (True, False):
        Y32, Z32 = eng.pool_apply(0, imp, center, V, want_scores=True)
        Y5, Z5 = eng.pool_apply(0, imp, center, V[idx], want_scores=True)
        _bits(Z5, Z32[:, idx], f"scores imp={imp}")
        _bits(Y5, Y32[idx], f"Y imp={imp}")
        Y1, Z1 = eng.pool_apply(0, imp, center, V[3:4], want_scores=True)      # direction 3 of r = 32 == direction 0 of r = 1
        _bits(Z1[:, 0], Z32[:, 3])
        _bits(Y1[0], Y32[3])
        _bits(eng.pool_apply(0, imp, center, V[idx], carry=X[idx]), eng.pool_apply(0, imp, center, V, carry=X)[idx], f"carry imp={imp}")
    assert not np.array_equal(Y32[0], Y32[1])


@pytest.mark.parametrize("name,N_r,r", [("lr65", 37, 5), ("d130", 37, 17), ("lr10", 1000, 16), ("d1000", 5, 32)])
def test_carry(pfmi_mod, eng, name, N_r, r):
    """a random carry stays within the bound with M + 1 terms; runs {0, 1, 2} in one call == run {0}, then runs {1, 2} with the first
    result as the carry (the engine rebuilt; it keeps the PSIS weights of the K = 3 pool): the same bits"""
    P3, lr3 = _pool(pfmi_mod, eng, name, 3, N_r)
    d = P3.shape[0]
    w = eng.psis(lr3)["weights"]
    center = P3[:, 0, 2] * 0.5 + 0.1
    V = _dirs(5, r, d)
    X = np.random.default_rng(3).normal(size=(r, d)) * 10.0
    got, Z = eng.pool_apply(0, True, center, V, carry=X, want_scores=True)
    ref, A = pool_apply(P3, w, center, Z, X)
    _check("Y", f"{name} carry", got, ref, bound(3 * N_r + 1, A))
    whole = {imp: eng.pool_apply(0, imp, center, V, want_scores=True) for imp in (True, False)}
    _pool(pfmi_mod, eng, name, 1, N_r, runs=[0])
    first = {imp: eng.pool_apply(0, imp, center, V, want_scores=True) for imp in (True, False)}
    P12, _ = _pool(pfmi_mod, eng, name, 2, N_r, runs=[1, 2])
    np.testing.assert_array_equal(P12, P3[:, :, 1:])              # (precondition: the same draws)
    for imp in (True, False):
        Y, Z12 = eng.pool_apply(N_r, imp, center, V, carry=first[imp][0], want_scores=True)
        _bits(Y, whole[imp][0], f"imp={imp}")
        _bits(np.concatenate([first[imp][1], Z12]), whole[imp][1], f"scores imp={imp}")     # a score does not depend on K or the run's position
    assert not np.array_equal(eng.pool_apply(N_r, True, center, V), whole[True][0])         # (without the carry: another answer)


def test_col_offset_into_a_longer_psis_vector(pfmi_mod, eng):
    N_r, K, r = 37, 3, 5
    P, lr = _pool(pfmi_mod, eng, "lr65", K, N_r)
    rng = np.random.default_rng(8)
    off = 2 * N_r + 5
    glob = np.concatenate([rng.normal(size=off) + lr.mean(), lr, rng.normal(size=50) + lr.mean()])
    w = eng.psis(glob)["weights"]
    V = _dirs(9, r, P.shape[0])
    got, Z = eng.pool_apply(off, True, None, V, want_scores=True)
    Zr, Az = pool_scores(P, w[off:off + K * N_r], None, V)
    _check("scores", "col_offset", Z, Zr, bound_scores(P.shape[0], Az))
    ref, A = pool_apply(P, w[off:off + K * N_r], None, Z)
    _check("Y", "col_offset", got, ref, bound(K * N_r, A))
    assert not np.array_equal(eng.pool_apply(0, True, None, V), got)   # another window of the weights: another answer


def test_zero_weights_are_skipped(pfmi_mod, eng):
    N_r, K, r = 37, 3, 5
    P, lr = _pool(pfmi_mod, eng, "diag30", K, N_r)
    d = P.shape[0]
    lr = lr.copy()
    lr[N_r + 3:2 * N_r + 9] = -np.inf                            # a block across two runs
    lr[0] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.all(w[N_r + 3:2 * N_r + 9] == 0.0) and w[0] == 0.0 and np.count_nonzero(w) >= N_r
    center = P[:, 1, 1] + 0.25
    V = _dirs(2, r, d)
    for c in (None, center):
        _, Z = _parity(f"zero weights center={'y' if c is not None else 'n'}", eng, P, w, c, V)
        _bits(Z[w == 0.0], np.zeros((np.count_nonzero(w == 0.0), r)))      # the scores of skipped columns are exactly 0
        assert np.all(Z[w != 0.0] != 0.0)
    # a run whose columns all have weight 0 changes nothing: the output is the carry
    _pool(pfmi_mod, eng, "diag30", 1, N_r, runs=[1])
    lr[N_r:2 * N_r] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.all(w[N_r:2 * N_r] == 0.0)
    X = np.random.default_rng(4).normal(size=(r, d))
    Y, Z = eng.pool_apply(N_r, True, center, V, carry=X, want_scores=True)
    _bits(Y, X)
    _bits(Z, np.zeros((N_r, r)))
    _bits(eng.pool_apply(N_r, True, center, V), np.zeros((r, d)))


@pytest.mark.parametrize("name,r", [("lr10", 5), ("lr65", 17), ("d130", 16), ("d1000", 5)])
def test_nan_under_a_zero_weight_is_invisible_and_under_a_weight_poisons_its_scores_and_all_of_y(pfmi_mod, eng, name, r):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    z, c = N_r + 20, 2 * N_r + 36                                  # columns of runs 1 and 2 (the ragged last group of run 2)
    r0, r1 = d // 2, d - 1
    lr = lr.copy()
    lr[z] = -np.inf
    w = eng.psis(lr)["weights"]
    assert w[z] == 0.0 and w[c] != 0.0
    center = P[:, 0, 0] * 0.5
    V = _dirs(6, r, d)
    V[0, r0] = V[0, r1] = 0.0                                     # a zero of a direction against the NaN: NaN all the same
    baseY, baseZ = eng.pool_apply(0, True, center, V, want_scores=True)
    uniY, uniZ = eng.pool_apply(0, False, center, V, want_scores=True)
    assert np.all(np.isfinite(baseY)) and np.all(np.isfinite(baseZ)) and np.all(np.isfinite(uniZ))
    ptr, count = eng.pool_draws_dev()
    assert count == d * K * N_r
    nan = np.array([np.nan])

    eng.memcpy_h2d(ptr + 8 * (z * d + r0), nan)                    # under a zero weight: invisible
    Pn = eng.pool_get()[0]
    assert np.isnan(Pn[r0, z % N_r, z // N_r]) and np.count_nonzero(np.isnan(Pn)) == 1
    Y, Z = eng.pool_apply(0, True, center, V, want_scores=True)
    _bits(Y, baseY)
    _bits(Z, baseZ)
    Y, Z = eng.pool_apply(0, False, center, V, want_scores=True)   # unit weights skip nothing: that column's scores and all of Y
    bad = np.zeros(Z.shape, dtype=bool)
    bad[z] = True
    np.testing.assert_array_equal(np.isnan(Z), bad)
    _bits(Z[~bad], uniZ[~bad])
    assert np.all(np.isnan(Y))

    eng.memcpy_h2d(ptr + 8 * (c * d + r1), nan)                    # under a non-zero weight
    Y, Z = eng.pool_apply(0, True, center, V, want_scores=True)
    bad = np.zeros(Z.shape, dtype=bool)
    bad[c] = True
    np.testing.assert_array_equal(np.isnan(Z), bad)
    _bits(Z[~bad], baseZ[~bad])                                    # every other score has the bits of the clean run
    assert np.all(np.isnan(Y))


def test_error_codes(pfmi_mod):
    def then(e):
        d = e.d
        V, out = np.ones((33, d)), np.empty((33, d))
        p = lambda a: a.ctypes.data_as(pfmi_mod._lib._dp)         # noqa: E731
        L = e.L
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 1, p(V), None, p(out), None) == 0
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 32, p(V), None, p(out), None) == 0
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 0, p(V), None, p(out), None) == -1       # r = 0
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 33, p(V), None, p(out), None) == -1      # r = 33
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, -1, p(V), None, p(out), None) == -1
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 2, None, None, p(out), None) == -1       # v NULL
        assert L.pfmi_pool_apply(e.ctx, 0, 0, None, 2, p(V), None, None, None) == -1         # y_out NULL
        with pytest.raises(pfmi_mod.PfmiError) as ex:
            e.pool_apply(0, False, None, V)
        assert ex.value.code == -1
        for bad in (dict(V=None), dict(V=np.ones(d)), dict(V=np.ones((2, d + 1))), dict(V=np.ones((2, d)), center=np.zeros(3)),
                    dict(V=np.ones((2, d)), carry=np.zeros((3, d))), dict(V=np.ones((2, d)), carry=np.zeros(2 * d))):
            with pytest.raises(ValueError):
                e.pool_apply(0, False, **bad)

    check_pool_error_codes(pfmi_mod, lambda e, off, imp: e.pool_apply(off, imp, None, np.ones((2, e.d))), then)


@pytest.mark.parametrize("d,r", [(10, 3), (65, 8)])
def test_lowrank_covariance_of_a_multipathfinder_result(pfmi_mod, d, r):
    """lowrank_covariance(4) against eigh of covariance().cov, the dense matrix of the same pool.  With M = K N_r, n = M + 5 and A the
    absolute sums of the cross moments about the mean, the dense matrix is entrywise within 2 (n + 1) u max A / W of the exact covariance
    (test_gpu_pool_cross); the operator the iteration applies is the same sums contracted in two steps, each entry of it within
    (2 (n + 1) + d + 4) u max A / W (the scores add (d + 4) u relative to their absolute sums).  A spectral norm is at most d times the
    largest entry, so the two operators differ by at most E = d (4 (n + 1) + d + 4) u max A / W in norm, and by Weyl's inequality so do
    their eigenvalues.  So: every returned lam_j lies within rho_j + 64 u d lam_1 + E of an eigenvalue of the dense matrix (the residual
    inclusion theorem, the slack of the CPU test for the host algebra, E), and |dense() - cov|_2 <= lam_{rank+1}(cov) + max rho_j + the
    same slack."""
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        tg = pfmi.t_lowrank(d, r=r, seed=2)
        res = pfmi.multipathfinder(tg, 100, nruns=3, ndraws_per_run=50, rng=pfmi.HostRNG(4), engine=e)
        K, N_r, rank = 3, 50, 4
        P = None
        for imp in (True, False):
            lr = res.lowrank_covariance(rank, importance=imp)
            assert isinstance(lr, pfmi.LowRankCovariance) and lr.ncandidates == K * N_r
            if P is None:
                P = np.array(e.pool_get()[0])                    # the pool the call rebuilt
                np.testing.assert_array_equal(P, np.stack([x.draws for x in res.pathfinder_results], axis=2))
            c = res.covariance(importance=imp)
            s = res.summary(importance=imp)
            _bits(lr.mean, s.mean)
            _bits(lr.var, s.var)
            assert lr.ess == s.ess and (lr.pareto_shape == c.pareto_shape or not imp)
            assert lr.converged and 1 <= lr.passes <= 30
            assert lr.eigenvalues.shape == (rank,) and lr.eigenvectors.shape == (d, rank) and np.all(lr.diag >= 0)
            ref = covariance(P, res.psis_result.weights if imp else None)
            n = K * N_r + 5
            E = float(d * (4 * (n + 1) + d + 4) * U * np.max(ref["A"]) / ref["W"])
            ev = np.linalg.eigvalsh(c.cov)
            slack = 64 * 2.0 ** -53 * d * ev[-1] + E
            ratios = [float(np.min(np.abs(ev - lr.eigenvalues[j])) / (lr.residuals[j] + slack)) for j in range(rank)]
            print(f"lowrank_covariance d={d} imp={int(imp)}: passes={lr.passes} residuals={lr.residuals} eigenvalues={lr.eigenvalues} "
                  f"worst |lam - eig| / (rho + slack) = {max(ratios):.3g}")
            mg.check("pool_apply", "eigenvalues", max(ratios), bound=1.0, contract=1.0, ctx=f"d={d} imp={int(imp)}")
            gap = float(np.linalg.norm(lr.dense() - c.cov, 2) / (ev[::-1][rank] + np.max(lr.residuals) + slack))
            print(f"lowrank_covariance d={d} imp={int(imp)}: |dense() - cov|_2 / (lam_(rank+1) + max rho + slack) = {gap:.3g}")
            mg.check("pool_apply", "dense_vs_cov", gap, bound=1.0, contract=1.0, ctx=f"d={d} imp={int(imp)}")
            np.testing.assert_allclose(np.diagonal(lr.dense()), np.maximum(lr.var, (lr.eigenvectors ** 2) @ lr.eigenvalues), rtol=1e-12)
            if np.all(lr.diag > 0):
                x = np.random.default_rng(1).normal(size=d)
                assert np.linalg.norm(lr.dense() @ lr.solve(x) - x) <= 1e-10 * np.linalg.norm(x) * np.linalg.cond(lr.dense())
        again = pfmi.importance_lowrank_covariance(res, rank)
        first = res.lowrank_covariance(rank)
        for f in ("mean", "var", "eigenvalues", "eigenvectors", "diag", "residuals"):
            _bits(getattr(again, f), getattr(first, f), f)
        for bad in (0, min(d, 32) + 1):
            with pytest.raises(ValueError):
                res.lowrank_covariance(bad)
        e.fit_batch(J)                                           # the engine is refitted: the stored handles are stale
        with pytest.raises(pfmi.StaleHandleError):
            res.lowrank_covariance(rank)
    finally:
        e.close()


def test_a_nan_draw_under_a_weight_is_a_value_error(pfmi_mod, eng):
    """the host iteration on top of the primitive: a NaN in a counted column is named, not iterated on"""
    from pfmi.api import _lowrank_from_apply
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "lr10", K, N_r)
    d = P.shape[0]
    eng.psis(lr)
    ptr, _ = eng.pool_draws_dev()
    eng.memcpy_h2d(ptr + 8 * (5 * d + 2), np.array([np.nan]))
    with pytest.raises(ValueError, match="not finite"):
        _lowrank_from_apply(lambda Q: eng.pool_apply(0, False, None, np.ascontiguousarray(Q.T)).T, d, 2)


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
V = np.random.default_rng(0).normal(size=(17, 65))
for imp in (True, False):
    a, b = (pfmi.importance_lowrank_covariance(r, 4, importance=imp) for r in (one, two))
    for f in ("mean", "var", "eigenvalues", "eigenvectors", "diag", "residuals"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (imp, f)
    assert a.passes == b.passes and a.converged and b.converged and a.ess == b.ess, imp
    assert np.all(np.isfinite(a.eigenvectors)) and np.all(a.eigenvalues > 0)
    # the primitive over the two engines, chained through the carry, has the bits of the one engine
    off = len(two.pathfinder_results) // 2 * 50
    y0, z0 = one.engine.pool_apply(0, imp, a.mean, V, want_scores=True)
    y1, z1 = engs[0].pool_apply(0, imp, a.mean, V, want_scores=True)
    y2, z2 = engs[1].pool_apply(off, imp, a.mean, V, carry=y1, want_scores=True)
    assert np.array_equal(y2, y0) and not np.array_equal(y1, y0)
    assert np.array_equal(np.concatenate([z1, z2]), z0)
print("lowrank engines ok")
"""


@pytest.mark.timeout(600)
def test_lowrank_covariance_over_two_engines_is_bit_identical():
    """engines=[Engine(0), Engine(0)] through the RCCL stand-in: the low-rank covariance and the chained primitive have the bits of the
    one-engine result"""
    run_two_engines(_MULTI, "lowrank engines ok")
