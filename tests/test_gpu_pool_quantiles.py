"""Weighted CDF of the pool on the device (pfmi_pool_cdf / Engine.pool_cdf) and the importance quantiles searched on it
(pfmi.importance_quantiles, MultiPathfinderResult.quantiles).

Primitive: pool_build, pool_get + psis, pool_cdf; compared with the longdouble reference (tests/pool_quantiles_reference.py) on the
DOWNLOADED pool and weights.  below / above / nanflag must be equal exactly; |wle - ref| <= (K N_r + 5) 2^-53 * (sum of the counted
weights): any order of adding K N_r non-negative terms is within (K N_r - 1) u of the exact sum relative to the sum of all terms,
the same form as the moments' bound.  The worst ratio is recorded through tests/margins.py (config "pool_quantiles").  Shapes are those
of tests/pool_common.py (CASES), at which the kernels' paths switch; threshold counts 3, 8, 13 and 32 take every instantiation
(4, 8, 16 thresholds per thread, two rows per lane up to 8, the doubled workgroup above 16).

NaN rules: a NaN is written into the pool on the device through pfmi_pool_draws_dev + pfmi_memcpy_h2d, under a zero and under a
non-zero weight, at shapes with several slots per workgroup (d < 64, d = 65), with one (d = 1000) and at every instantiation."""
import numpy as np
import pytest

import margins as mg
from pool_common import CASES, LD, U, J, _pool, check_pool_error_codes, run_two_engines
from pool_quantiles_reference import cdf, quantiles

pytestmark = pytest.mark.gpu

NTHR = (3, 8, 13, 32)
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def _thresholds(P2, seed):
    """32 thresholds per row of the flattened pool P2 (d, S): -inf, +inf, a pool value itself, a value between two neighbours (the
    pool value again when the row has one value), three equal thresholds, then values spread over the row's range and beyond"""
    d, S = P2.shape
    rng = np.random.default_rng(seed)
    srt = np.sort(P2, axis=1)
    a, b = srt[:, (S - 1) // 2], srt[:, min((S - 1) // 2 + 1, S - 1)]
    lo, hi = srt[:, 0], srt[:, -1]
    T = np.empty((32, d))
    T[0], T[1], T[2], T[3] = -np.inf, np.inf, P2[:, S // 3], a + (b - a) * 0.5
    T[4] = T[5] = T[6] = P2[:, S // 2]
    T[7:] = lo - 0.1 * (hi - lo) - 1e-3 + rng.uniform(size=(25, d)) * (1.2 * (hi - lo) + 2e-3)
    return T


def _check_cdf(tag, got, ref, n_terms, total):
    wle, below, above, nanflag = got
    np.testing.assert_array_equal(below, ref["below"][:below.shape[0]], err_msg=tag)
    np.testing.assert_array_equal(above, ref["above"][:above.shape[0]], err_msg=tag)
    np.testing.assert_array_equal(nanflag, ref["nanflag"], err_msg=tag)
    err = np.abs(wle.astype(LD) - ref["wle"][:wle.shape[0]])
    ratio = float(np.max(err / ((n_terms + 5) * U * total)))
    print(f"pool_cdf {tag}: worst |wle - ref| / bound = {ratio:.3g}")
    mg.check("pool_quantiles", "wle", ratio, bound=1.0, contract=1.0, ctx=tag)


@pytest.mark.parametrize("name,N_r,K", CASES, ids=[f"{n}-N{r}-K{k}" for n, r, k in CASES])
def test_pool_cdf_matches_the_longdouble_reference(pfmi_mod, eng, name, N_r, K):
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    P2 = P.reshape(d, K * N_r, order="F")
    w = eng.psis(lr)["weights"]
    T = _thresholds(P2, d + N_r)
    for imp in (True, False):
        ref = cdf(P2, w if imp else None, T)
        total = w[w != 0].astype(LD).sum() if imp else LD(K * N_r)
        for n in NTHR:
            got = eng.pool_cdf(0, imp, T[:n])
            assert got[0].shape == (n, d) and got[3].shape == (d,) and got[3].dtype == np.int32
            _check_cdf(f"{name} N_r={N_r} K={K} imp={int(imp)} nthr={n}", got, ref, K * N_r, total)
            if not imp:                                          # unit weights: the integer counts exactly
                np.testing.assert_array_equal(got[0], ref["wle"][:n].astype(np.float64))
        assert np.all(got[1][0] == -np.inf) and np.all(got[2][1] == np.inf)          # nothing at or below -inf / above +inf


@pytest.mark.parametrize("name,N_r", [("lr65", 37), ("d1000", 37), ("lr10", 1000), ("d130", 37)])
def test_carry_chains_contexts_in_run_order(pfmi_mod, eng, name, N_r):
    """runs {0, 1, 2} on one engine == runs {0, 1}, then run {2} with the first result as the carry (the engine rebuilt; it keeps the
    PSIS weights of the K = 3 pool): the same bits, for every instantiation"""
    P3, lr3 = _pool(pfmi_mod, eng, name, 3, N_r)
    d = P3.shape[0]
    P2 = P3.reshape(d, 3 * N_r, order="F")
    w = eng.psis(lr3)["weights"]
    T = _thresholds(P2, 5)
    whole = {(imp, n): eng.pool_cdf(0, imp, T[:n]) for imp in (True, False) for n in NTHR}
    again = eng.pool_cdf(0, True, T)
    for x, y in zip(whole[(True, 32)], again):
        np.testing.assert_array_equal(x, y)
    _pool(pfmi_mod, eng, name, 2, N_r, runs=[0, 1])
    first = {key: eng.pool_cdf(0, key[0], T[:key[1]]) for key in whole}
    _pool(pfmi_mod, eng, name, 1, N_r, runs=[2])
    for (imp, n), a in whole.items():
        f = first[(imp, n)]
        s = eng.pool_cdf(2 * N_r, imp, T[:n], carry=f[0])
        np.testing.assert_array_equal(s[0], a[0], err_msg=f"wle imp={imp} nthr={n}")
        np.testing.assert_array_equal(np.maximum(f[1], s[1]), a[1])
        np.testing.assert_array_equal(np.minimum(f[2], s[2]), a[2])
        np.testing.assert_array_equal(f[3] | s[3], a[3])
    assert not np.array_equal(eng.pool_cdf(2 * N_r, True, T)[0], whole[(True, 32)][0])      # (without the carry: another answer)


def test_col_offset_into_a_longer_psis_vector(pfmi_mod, eng):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "lr65", K, N_r)
    P2 = P.reshape(P.shape[0], K * N_r, order="F")
    rng = np.random.default_rng(8)
    off = 2 * N_r + 5
    glob = np.concatenate([rng.normal(size=off) + lr.mean(), lr, rng.normal(size=50) + lr.mean()])
    w = eng.psis(glob)["weights"]
    T = _thresholds(P2, 6)
    wl = w[off:off + K * N_r]
    got = eng.pool_cdf(off, True, T)
    _check_cdf("col_offset", got, cdf(P2, wl, T), K * N_r, wl[wl != 0].astype(LD).sum())
    assert not np.array_equal(eng.pool_cdf(0, True, T)[0], got[0])


def test_zero_weights_are_skipped(pfmi_mod, eng):
    """a zero-weight column enters neither the sums nor below / above: the run of the row's extreme values gets weight 0"""
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "diag30", K, N_r)
    P2 = P.reshape(P.shape[0], K * N_r, order="F")
    lr = lr.copy()
    lr[np.argmax(P2[0])] = -np.inf
    lr[np.argmin(P2[0])] = -np.inf
    lr[N_r + 3:2 * N_r + 9] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.count_nonzero(w == 0) >= N_r + 6
    T = _thresholds(P2, 7)
    got = eng.pool_cdf(0, True, T)
    _check_cdf("zero weights", got, cdf(P2, w, T), K * N_r, w[w != 0].astype(LD).sum())
    assert got[1][1][0] < P2[0].max() and got[2][0][0] > P2[0].min()


@pytest.mark.parametrize("name", ["lr10", "diag30", "lr65", "d130", "d1000"])
def test_nan_under_a_zero_weight_is_invisible_and_under_a_weight_sets_the_flag(pfmi_mod, eng, name):
    from pfmi.api import _quantiles_of_pool
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    P2 = P.reshape(d, K * N_r, order="F")
    z, c = N_r + 20, 2 * N_r + 36                                  # columns of runs 1 and 2 (second chunks where a run has two)
    r0, r1 = d // 2, d - 1                                         # (d - 1: the second row of a lane's pair where lanes hold two)
    lr = lr.copy()
    lr[z] = -np.inf
    w = eng.psis(lr)["weights"]
    assert w[z] == 0.0 and w[c] != 0.0
    T = _thresholds(P2, 9)
    base = {n: eng.pool_cdf(0, True, T[:n]) for n in NTHR}
    qbase, _ = _quantiles_of_pool([eng], [(0, K)], N_r, True, np.array(PROBS))
    assert np.all(np.isfinite(qbase))
    ptr, count = eng.pool_draws_dev()
    assert count == d * K * N_r
    nan = np.array([np.nan])

    eng.memcpy_h2d(ptr + 8 * (z * d + r0), nan)                    # under a zero weight: invisible
    Pn = eng.pool_get()[0].reshape(d, K * N_r, order="F")
    P2[r0, z] = np.nan
    np.testing.assert_array_equal(Pn, P2)
    for n in NTHR:
        got = eng.pool_cdf(0, True, T[:n])
        for x, y in zip(got, base[n]):
            np.testing.assert_array_equal(x, y, err_msg=f"zero weight nthr={n}")
        assert not got[3].any()
        uni = eng.pool_cdf(0, False, T[:n])                        # unit weights skip nothing: the flag of that row alone
        ref = cdf(P2, None, T[:n])
        np.testing.assert_array_equal(uni[3], np.arange(d) == r0)
        _check_cdf(f"{name} NaN unweighted nthr={n}", uni, ref, K * N_r, LD(K * N_r))
        np.testing.assert_array_equal(uni[0], ref["wle"].astype(np.float64))
    q, _ = _quantiles_of_pool([eng], [(0, K)], N_r, True, np.array(PROBS))
    np.testing.assert_array_equal(q, qbase)

    eng.memcpy_h2d(ptr + 8 * (c * d + r1), nan)                    # under a non-zero weight: the flag, and nothing else changes
    P2[r1, c] = np.nan
    others = np.arange(d) != r1
    for n in NTHR:
        got = eng.pool_cdf(0, True, T[:n])
        np.testing.assert_array_equal(got[3], (~others).astype(np.int32), err_msg=f"nthr={n}")
        _check_cdf(f"{name} NaN weighted nthr={n}", got, cdf(P2, w, T[:n]), K * N_r, w[w != 0].astype(LD).sum())
        for x, y in zip(got[:3], base[n][:3]):
            np.testing.assert_array_equal(x[:, others], y[:, others], err_msg=f"other rows nthr={n}")
    q, _ = _quantiles_of_pool([eng], [(0, K)], N_r, True, np.array(PROBS))
    assert np.all(np.isnan(q[:, r1]))
    np.testing.assert_array_equal(q[:, others], qbase[:, others])


def test_error_codes(pfmi_mod):
    T = np.zeros((4, 10))

    def then(e):
        for bad in (np.zeros((0, 10)), np.zeros((33, 10))):      # nthr outside [1, 32]
            with pytest.raises(pfmi_mod.PfmiError) as ex:
                e.pool_cdf(0, False, bad)
            assert ex.value.code == -1
        for bad in (np.zeros((4, 9)), np.zeros(40)):             # a wrong thresholds length
            with pytest.raises(ValueError):
                e.pool_cdf(0, False, bad)
        with pytest.raises(ValueError):
            e.pool_cdf(0, False, T, carry=np.zeros((3, 10)))

    check_pool_error_codes(pfmi_mod, lambda e, off, imp: e.pool_cdf(off, imp, T), then)


def _check_quantiles(tag, q, P2, w, W, probs):
    """with importance weighting: equal to the reference wherever its margin exceeds tau = 2 (S + 5) 2^-53 W; elsewhere the value
    must itself satisfy the definition within tau.  The share of such entries is asserted on the reference's margins alone."""
    S = P2.shape[1]
    ref, margin = quantiles(P2, w, probs, W)
    tau = 2 * (S + 5) * U * LD(W)
    safe = margin > tau
    print(f"importance_quantiles {tag}: smallest margin / tau = {float(margin.min() / tau):.3g}, entries within tau: {int((~safe).sum())}")
    assert safe.all(), (tag, float(margin.min() / tau))
    np.testing.assert_array_equal(q[safe], ref[safe], err_msg=tag)


def test_importance_quantiles_of_a_multipathfinder_result(pfmi_mod):
    pfmi = pfmi_mod
    from pfmi.api import CDF_THRESHOLDS_PER_PASS, _quantile_pass_cap
    e = pfmi.Engine(0)
    try:
        tg = pfmi.t_lowrank(50, r=8, seed=2)
        res = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4), engine=e)
        P = np.stack([r.draws for r in res.pathfinder_results], axis=2)
        P2 = P.reshape(50, -1, order="F")
        w = res.psis_result.weights
        q, passes = pfmi.importance_quantiles(res, return_passes=True)
        cap = _quantile_pass_cap(CDF_THRESHOLDS_PER_PASS // len(PROBS))
        print(f"importance_quantiles: {passes} passes (cap {cap})")
        assert q.shape == (5, 50) and passes <= cap
        np.testing.assert_array_equal(res.quantiles(), q)
        W = pfmi.api._combine_moments([e.pool_moments(0, True, None)[0]])[0]           # the W the search formed its targets with
        _check_quantiles("weighted", q, P2, w, W, PROBS)
        for i in range(50):
            assert np.all(np.isin(q[:, i], P2[i]))
        probs = (0.0, 0.1, 0.5, 1.0)
        u, pu = pfmi.importance_quantiles(res, probs, importance=False, return_passes=True)
        print(f"importance_quantiles uniform: {pu} passes")
        np.testing.assert_array_equal(u, np.quantile(P2, probs, axis=1, method="inverted_cdf"))
        np.testing.assert_array_equal(res.quantiles(PROBS, importance=False), np.quantile(P2, PROBS, axis=1, method="inverted_cdf"))
        # more probabilities than one pass holds: the same answers
        many = np.linspace(0.05, 0.95, 19)
        np.testing.assert_array_equal(res.quantiles(many, importance=False), np.quantile(P2, many, axis=1, method="inverted_cdf"))
        s = res.summary()                                        # summary() is unchanged by the shared preamble
        assert np.all(q[0] <= s.mean + 10 * s.std) and np.all(q[4] >= s.mean - 10 * s.std)
        with pytest.raises(ValueError):
            res.quantiles((0.5, 1.5))
        e.fit_batch(J)                                           # the engine is refitted: the stored handles are stale
        with pytest.raises(pfmi.StaleHandleError):
            res.quantiles()
    finally:
        e.close()


_MULTI = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/pathfinder.jl_amd")
import pfmi
tg = pfmi.t_lowrank(50, r=8, seed=2)
one = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4))
engs = [pfmi.Engine(0), pfmi.Engine(0)]
two = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4), engines=engs)
assert len({id(r.fit_distribution.engine) for r in two.pathfinder_results}) == 2
for imp in (True, False):
    (a, pa), (b, pb) = (pfmi.importance_quantiles(r, importance=imp, return_passes=True) for r in (one, two))
    assert np.array_equal(a, b) and pa == pb, (imp, pa, pb, np.max(np.abs(a - b)))
    # the primitive over the two engines, chained through the carry, has the bits of the one engine
    T = np.stack([a[2], a[0], np.full(50, np.inf)])
    off = len(two.pathfinder_results) // 2 * 50
    w0 = one.engine.pool_cdf(0, imp, T)
    w1 = engs[0].pool_cdf(0, imp, T)
    w2 = engs[1].pool_cdf(off, imp, T, carry=w1[0])
    assert np.array_equal(w2[0], w0[0]) and np.array_equal(np.maximum(w1[1], w2[1]), w0[1]) and np.array_equal(np.minimum(w1[2], w2[2]), w0[2])
print("quantiles engines ok", pa)
"""


@pytest.mark.timeout(600)
def test_quantiles_over_two_engines_are_bit_identical():
    """engines=[Engine(0), Engine(0)] through the RCCL stand-in: quantiles, pass count and the chained primitive have the bits of the
    one-engine result"""
    run_two_engines(_MULTI, "quantiles engines ok")
