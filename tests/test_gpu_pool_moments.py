"""Weighted moments of the pool on the device (pfmi_pool_moments / Engine.pool_moments) and the importance summaries built on them
(pfmi.importance_summary, MultiPathfinderResult.summary).

Sequence of every kernel case: pool_build, pool_get + psis, pool_moments; the result is compared with the longdouble restatement of
the formulas (tests/pool_moments_reference.py) on the DOWNLOADED pool and weights.  Bound per entry, derived, not tuned:
|gpu - ref| <= (N_r + 4) 2^-53 A, A the sum of the absolute values of the entry's terms (pool_moments_reference.bound).  The worst
observed ratio to the bound is recorded through tests/margins.py (config "pool_moments") and printed.

Shapes: tests/pool_common.py (CASES), every size at which the column walk takes another path; K = 1, 3."""
import numpy as np
import pytest

import margins as mg
from pool_common import CASES, LD, U, J, _pool, check_pool_error_codes, ratio_to_bound, run_two_engines
from pool_moments_reference import bound, pool_moments, summary

pytestmark = pytest.mark.gpu


def _check(tag, got, ref, N_r):
    wsum, s1, s2, s2w = got
    worst = {}
    for q, g, r, a in (("wsum", wsum, ref["wsum"], ref["Aw"]), ("s1", s1, ref["s1"], ref["A1"]), ("s2", s2, ref["s2"], ref["A2"]),
                       ("s2w", s2w, ref["s2w"], ref["A2w"])):
        assert g.shape == r.shape, (tag, q, g.shape, r.shape)
        worst[q] = ratio_to_bound(bound, g, r, a, N_r)
    print(f"pool_moments {tag}: worst |gpu - ref| / bound = " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():                                 # (printed for every quantity before the first assertion)
        mg.check("pool_moments", q, v, bound=1.0, contract=1.0, ctx=tag)


@pytest.mark.parametrize("name,N_r,K", CASES, ids=[f"{n}-N{r}-K{k}" for n, r, k in CASES])
def test_pool_moments_match_the_longdouble_reference(pfmi_mod, eng, name, N_r, K):
    P, lr = _pool(pfmi_mod, eng, name, K, N_r)
    d = P.shape[0]
    w = eng.psis(lr)["weights"]
    center = np.random.default_rng(d + N_r).normal(size=d) * 0.7 + P[:, 0, 0]
    for imp in (True, False):
        for c in (None, center):
            got = eng.pool_moments(0, imp, c)
            assert got[0].shape == (K, 2) and got[1].shape == (K, d)
            ref = pool_moments(P, w if imp else None, c)
            _check(f"{name} N_r={N_r} K={K} imp={int(imp)} center={'y' if c is not None else 'n'}", got, ref, N_r)
    if not imp:
        np.testing.assert_array_equal(got[0], np.full((K, 2), float(N_r)))        # uniform: sum w = sum w^2 = N_r exactly


def test_col_offset_into_a_longer_psis_vector(pfmi_mod, eng):
    """the local pool is columns [off, off + K N_r) of a global pool whose PSIS the engine holds"""
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "lr65", K, N_r)
    rng = np.random.default_rng(8)
    off = 2 * N_r + 5
    glob = np.concatenate([rng.normal(size=off) + lr.mean(), lr, rng.normal(size=50) + lr.mean()])
    w = eng.psis(glob)["weights"]
    got = eng.pool_moments(off, True, None)
    _check("col_offset", got, pool_moments(P, w[off:off + K * N_r], None), N_r)
    other = eng.pool_moments(0, True, None)                      # another window of the weights: another answer
    assert not np.array_equal(other[0], got[0])


def test_zero_weights_are_skipped(pfmi_mod, eng):
    N_r, K = 37, 3
    P, lr = _pool(pfmi_mod, eng, "diag30", K, N_r)
    lr = lr.copy()
    lr[N_r + 3:2 * N_r + 9] = -np.inf                            # a block across two runs
    lr[0] = -np.inf
    w = eng.psis(lr)["weights"]
    assert np.all(w[N_r + 3:2 * N_r + 9] == 0.0) and w[0] == 0.0 and np.count_nonzero(w) >= N_r
    center = P[:, 1, 1] + 0.25
    for c in (None, center):
        _check("zero weights", eng.pool_moments(0, True, c), pool_moments(P, w, c), N_r)
    # a run whose columns all have weight 0 gives exact zeros
    lr[:N_r] = -np.inf
    eng.psis(lr)
    got = eng.pool_moments(0, True, center)
    for a in got:
        np.testing.assert_array_equal(a[0], np.zeros_like(a[0]))


@pytest.mark.parametrize("name,N_r", [("lr65", 37), ("d1000", 37), ("lr10", 1000)])
def test_rows_do_not_depend_on_where_the_run_sits(pfmi_mod, eng, name, N_r):
    """the same fit pooled as run 2 of K = 3 and as run 0 of K = 1 (its weights then sit at col_offset = 2 N_r of the PSIS vector the
    engine still holds): bit-identical rows; and two calls return identical bits"""
    P3, lr3 = _pool(pfmi_mod, eng, name, 3, N_r)
    d = P3.shape[0]
    eng.psis(lr3)
    center = P3[:, 0, 2] * 0.5 + 0.1
    a_imp, a_uni = eng.pool_moments(0, True, center), eng.pool_moments(0, False, None)
    again = eng.pool_moments(0, True, center)
    for x, y in zip(a_imp, again):
        np.testing.assert_array_equal(x, y)
    P1, _ = _pool(pfmi_mod, eng, name, 1, N_r, runs=[2])           # the engine keeps the PSIS weights of the K = 3 pool
    np.testing.assert_array_equal(P1[:, :, 0], P3[:, :, 2])       # (precondition: the same draws)
    b_imp, b_uni = eng.pool_moments(2 * N_r, True, center), eng.pool_moments(0, False, None)
    for x, y in zip(a_imp, b_imp):
        np.testing.assert_array_equal(x[2], y[0])
    for x, y in zip(a_uni, b_uni):
        np.testing.assert_array_equal(x[2], y[0])
    assert b_imp[1].shape == (1, d)


def test_error_codes(pfmi_mod):
    def then(e):
        with pytest.raises(ValueError):
            e.pool_moments(0, False, np.zeros(3))

    check_pool_error_codes(pfmi_mod, lambda e, off, imp: e.pool_moments(off, imp, None), then)


def _summary_bounds(P, w):
    """reference summary of the pool and the bounds of its entries.  With n = N_r + K + 5: every per-run sum is within (N_r + 4) u of
    its absolute sum A, the host adds K of them ((K - 1) u more) and W = sum w carries the same relative error, so a quotient
    sum / W is within 2 n u A / W (one u for the division); var = s2 / W - (s1 / W)^2 does not depend on the centre, its second term
    is of the order of u^2, and the subtraction rounds once more: 2 (n + 1) u A2 / W; ess = W^2 / sum w^2 and run_weights are
    products / quotients of such sums: 3 n u and 2 n u relative."""
    d, N_r, K = P.shape
    ref = summary(P, w)
    m1 = pool_moments(P, w, None)
    m2 = pool_moments(P, w, np.asarray(ref["mean"], dtype=np.float64))
    W = m1["wsum"][:, 0].sum()
    n = N_r + K + 5
    return ref, dict(mean=2 * n * U * m1["A1"].sum(axis=0) / W, var=2 * (n + 1) * U * m2["A2"].sum(axis=0) / W,
                     ess=3 * n * U * ref["ess"], run_weights=2 * n * U * ref["run_weights"])


def _check_summary(tag, s, P, w):
    ref, bnd = _summary_bounds(P, w)
    # mcse_mean = sqrt(sum w^2 (x - c)^2) / W DOES depend on the centre: its reference is formed about the summary's own mean (2 n u
    # relative: the root halves the sum's n u, W adds n u, one u each for root and division)
    m = pool_moments(P, w, np.asarray(s.mean, dtype=np.float64))
    ref["mcse_mean"] = np.sqrt(m["s2w"].sum(axis=0)) / m["wsum"][:, 0].sum()
    bnd["mcse_mean"] = 2 * (P.shape[1] + P.shape[2] + 5) * U * ref["mcse_mean"]
    for q in ("mean", "var", "ess", "run_weights", "mcse_mean"):
        err = np.abs(np.asarray(getattr(s, q), dtype=LD) - ref[q])
        r = float(np.max(err / bnd[q]))
        print(f"importance_summary {tag}: {q} worst |gpu - ref| / bound = {r:.3g}")
        mg.check("pool_moments", f"summary_{q}", r, bound=1.0, contract=1.0, ctx=tag)
    np.testing.assert_array_equal(s.std, np.sqrt(s.var))
    assert abs(float(np.sum(s.run_weights)) - 1.0) <= float(2 * (P.shape[1] + 2 * P.shape[2] + 5) * U)
    assert s.ncandidates == P.shape[1] * P.shape[2]


def test_importance_summary_of_a_multipathfinder_result(pfmi_mod):
    pfmi = pfmi_mod
    e = pfmi.Engine(0)
    try:
        tg = pfmi.t_lowrank(50, r=8, seed=2)
        res = pfmi.multipathfinder(tg, 100, nruns=8, ndraws_per_run=50, rng=pfmi.HostRNG(4), engine=e)
        P = np.stack([r.draws for r in res.pathfinder_results], axis=2)
        w = res.psis_result.weights
        s = res.summary()
        assert isinstance(s, pfmi.ImportanceSummary) and s.pareto_shape == res.psis_result.pareto_shape
        _check_summary("weighted", s, P, w)
        flat = P.reshape(50, -1, order="F")
        np.testing.assert_allclose(s.mean, np.average(flat, axis=1, weights=w), rtol=1e-11, atol=1e-13)
        u = pfmi.importance_summary(res, importance=False)
        _check_summary("uniform", u, P, None)
        np.testing.assert_allclose(u.mean, flat.mean(axis=1), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(u.var, flat.var(axis=1), rtol=1e-11)
        assert u.ess == 400.0 and np.isnan(u.pareto_shape)
        np.testing.assert_array_equal(u.run_weights, np.full(8, 0.125))
        # the summary is a function of the stored candidates: an intervening resample with fresh candidates does not change it
        pfmi.resample(res, 100, ndraws_per_run=20)
        s2 = res.summary()
        for q in ("mean", "var", "std", "mcse_mean", "run_weights"):
            np.testing.assert_array_equal(getattr(s2, q), getattr(s, q))
        assert s2.ess == s.ess and s2.pareto_shape == s.pareto_shape and s2.ncandidates == 400
        e.fit_batch(J)                                           # the engine is refitted: the stored handles are stale
        with pytest.raises(pfmi.StaleHandleError):
            res.summary()
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
    a, b = one.summary(importance=imp), two.summary(importance=imp)
    for q in ("mean", "var", "std", "mcse_mean", "run_weights"):
        assert np.array_equal(getattr(a, q), getattr(b, q)), (imp, q, np.max(np.abs(getattr(a, q) - getattr(b, q))))
    assert a.ess == b.ess and a.ncandidates == b.ncandidates == 400, (imp, a.ess, b.ess)
    assert a.pareto_shape == b.pareto_shape or (np.isnan(a.pareto_shape) and np.isnan(b.pareto_shape))
print("summary engines ok", a.ess)
"""


@pytest.mark.timeout(600)
def test_summary_over_two_engines_is_bit_identical():
    """engines=[Engine(0), Engine(0)] through the RCCL stand-in: every field of summary() has the bits of the one-engine result"""
    run_two_engines(_MULTI, "summary engines ok")
