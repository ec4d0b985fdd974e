"""Pins the extended-precision per-draw reference of the ELBO scan (tests/scan_reference.py) against the double-precision oracle
(oracle/pf_oracle.c: Factor.rand_and_logpdf, GaussTarget.logp, FunnelTarget.logp, path_fit_elbo) on factors the oracle builds
itself, so that the GPU matrix (tests/test_gpu_scan_reference.py) compares the scan with a reference that is known to compute the
same quantities.  CPU only.

The oracle sums d terms in order and applies k reflectors, so it is within (d + 4 k + 16) eps S of the long-double value (S = the
reference's per-draw scale); the ELBO of N draws adds the mean of those bounds plus N eps |mean| from the oracle's pairwise sums."""
import numpy as np
import pytest

from oracle import pf_oracle as po
import scan_reference as sr

EPS = sr.EPS64


def _gauss(d, seed, r=0, spread=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    sig2 = np.exp(2 * spread * rng.uniform(-1, 1, d))
    a = 1 / sig2
    mean = rng.normal(size=d)
    if not r:
        return po.GaussTarget(mean, a, offset=offset)
    W = rng.normal(size=(d, r))
    Wd = W * a[:, None]
    G = np.linalg.inv(np.linalg.cholesky(np.eye(r) + W.T @ Wd))
    return po.GaussTarget(mean, a, np.asfortranarray(Wd), np.asfortranarray(G), offset)


def _fits(tg, J, seed=3, scale=2.0, maxiters=60):
    """an oracle L-BFGS trace of tg and its fits: [(l, j_eff, Factor, mu)], path_fit_elbo's result, the seeds"""
    x0 = np.random.default_rng(seed).uniform(-scale, scale, tg.d)
    P, _, G = po.optimize_trace(tg, x0, J, maxiters)
    alpha_all, hl, hs, _ = po.lbfgs_history(P, G, J)
    fits = []
    for l in range(1, len(P)):
        j = int(hl[l])
        S = np.stack([P[s + 1] - P[s] for s in hs[l, :j]], axis=1) if j else np.zeros((tg.d, 0))
        Y = np.stack([G[s] - G[s + 1] for s in hs[l, :j]], axis=1) if j else np.zeros((tg.d, 0))
        B, D = po.lbfgs_inverse_hessian(alpha_all[l], S, Y)
        F = po.Factor(alpha_all[l], B, D)
        if F.status == 0:
            fits.append((l, j, F, F.fit_mean(P[l], G[l])))
    return fits, P, G


def _compare(F, mu, tg, seed, N, n0=0, C_extra=0):
    """reference vs oracle for draws n0 .. n0 + N - 1 of one factor; returns the reference and the worst dev / (eps S) seen"""
    ref = sr.Ref(sr.LDFactor(F, mu), tg, seed, N, n0)
    U = po.randn_fill(seed, F.d, N, n0)
    X, lq = F.rand_and_logpdf(mu, U)
    lp = tg.logp(X)
    C = F.d + 4 * F.k + 16 + C_extra
    rp = np.abs(lp - ref.lp) / (EPS * ref.S_p)
    rq = np.abs(lq - ref.lq) / (EPS * ref.S_q)
    assert np.all(np.isfinite(ref.lp)) and np.all(np.isfinite(ref.S_p))
    assert rp.max() <= C and rq.max() <= C, (rp.max(), rq.max(), C)
    # the draws themselves (the oracle's x is what logp is evaluated at)
    xs = np.abs(np.asarray(F.sqrt_alpha)[:, None] * np.abs(U)).max() + np.abs(mu).max()
    assert np.max(np.abs(X - ref.X.astype(np.float64))) <= 64 * (F.k + 1) * EPS * xs * (1 + F.k)
    return ref, max(rp.max(), rq.max())


def _elbo_check(ref, elbo, se, N):
    tol = 4 * np.log2(N) * EPS * np.mean(np.abs(ref.lp - ref.lq)) + (ref.S_p.size + 64) * EPS * np.mean(ref.S_p + ref.S_q)
    assert abs(elbo - float(ref.elbo)) <= tol, (elbo, float(ref.elbo), tol)
    assert abs(se - float(ref.se)) <= tol + 1e-14 * float(ref.se), (se, float(ref.se))


def test_longdouble_is_extended():
    assert np.finfo(sr.LD).eps <= 1e-18


def test_j0_factor_is_diagonal():
    """j = 0 (no history: m = k = 0): x = mu + sqrt(alpha) u"""
    d = 37
    tg = _gauss(d, 1)
    rng = np.random.default_rng(5)
    F = po.Factor(rng.uniform(0.2, 3, d), np.zeros((d, 0)), np.zeros((0, 0)))
    mu = rng.normal(size=d)
    ref, _ = _compare(F, mu, tg, 77, 40)
    U = po.randn_fill(77, d, 40)
    np.testing.assert_allclose(ref.X.astype(np.float64), mu[:, None] + np.sqrt(F.alpha)[:, None] * U, rtol=1e-15, atol=1e-15)


@pytest.mark.parametrize("tname,d,r,J", [("diag", 30, 0, 6), ("lr", 50, 3, 6), ("lr", 40, 11, 8), ("lr", 64, 16, 5),
                                         ("lr10", 10, 3, 8), ("funnel", 12, 0, 6)])
def test_reference_matches_oracle_on_oracle_fits(tname, d, r, J):
    """every fit of an oracle trace: per-draw logp / logq within the oracle's own rounding of the long-double values, and the per-fit
    ELBO / SE of path_fit_elbo.  Covers k < 2J (the first fits read a partial ring), d < 2J (lr10: k = d = 10 < 16) and the
    diagonal, low-rank (r = 3, 11, 16) and funnel targets."""
    if tname == "funnel":
        tg = po.FunnelTarget(d)
    else:
        tg = _gauss(d, 2 + r, r)
    fits, P, G = _fits(tg, J, maxiters=25 if tname == "funnel" else 60)
    N = 64
    seeds = np.array([po.rand_u64(11, l, 9) for l in range(len(P))], dtype=np.uint64)
    o = po.path_fit_elbo(P, G, J, tg, N, seeds)
    ks = set()
    for l, j, F, mu in fits:
        ks.add(F.k)
        np.testing.assert_array_equal(mu, o["mu"][l])
        assert F.logdet == o["logdet"][l]
        ref, _ = _compare(F, mu, tg, int(seeds[l]), N)
        _elbo_check(ref, o["elbo"][l], o["se"][l], N)
    assert len(fits) >= 3
    assert min(ks) < 2 * J                                    # a partial ring (or d < 2J) was among the fits
    if d < 2 * J:
        assert max(ks) == d


def test_funnel_offset_draw_counters():
    """draws at n0 near 2^32: the reference reads the same wrapped counters as the oracle"""
    tg = po.FunnelTarget(9)
    fits, _, _ = _fits(tg, 4, maxiters=15)
    l, j, F, mu = fits[-1]
    for n0 in (0, 17, 2**32 - 5):
        _compare(F, mu, tg, 1234, 33, n0)
    a = sr.normals(1234, 9, 2**32 - 5, np.arange(10))
    np.testing.assert_array_equal(a[:, 5:], po.randn_fill(1234, 9, 5, 0))


def test_iso_identity_factor_analytic():
    """iso target, identity factor (alpha = 1, no history), mu = 0: x = u, logp = -|u|^2/2, logq = logp - d log(2 pi)/2, so every log
    ratio is d log(2 pi) / 2 and the ELBO is that with SE 0 -- in long double to its own precision"""
    d, N = 23, 50
    tg = po.GaussTarget(np.zeros(d), np.ones(d))
    F = po.Factor(np.ones(d), np.zeros((d, 0)), np.zeros((0, 0)))
    ref = sr.Ref(sr.LDFactor(F, np.zeros(d)), tg, 5, N)
    U = po.randn_fill(5, d, N).astype(sr.LD)
    half = d * sr.LOG2PI / 2
    usq = np.sum(U * U, axis=0)
    assert np.all(np.abs(ref.lp_ld + usq / 2) <= 8 * np.finfo(sr.LD).eps * usq)
    assert np.all(np.abs((ref.lp_ld - ref.lq_ld) - half) <= 64 * np.finfo(sr.LD).eps * (half + usq))
    assert abs(ref.elbo - half) <= 64 * np.finfo(sr.LD).eps * half and ref.se <= 1e-16
    assert abs(float(half) - 0.5 * d * np.log(2 * np.pi)) <= 4 * EPS * float(half)


def test_philox_words_and_miss_count():
    """the vectorised Philox of the reference is the oracle's (Random123 known answer at 10 rounds, the normal stream's 7), the miss
    threshold is the tail threshold of the table, and a counted miss is a normal from the tail refinement"""
    assert sr.MISS_BELOW == 1 << sr.ICDF_TAILBITS
    w = sr.philox_words(0, 0, 0, rounds=10)
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    seed = 0x1234_5678_9ABC_DEF0
    for n, g in ((0, 0), (5, 3), (2**32 - 1, 250)):
        exp = po.philox4x32([n, g, 0, 0], [seed & 0xFFFFFFFF, seed >> 32], sr.NORMAL_ROUNDS)
        assert [int(v) for v in sr.philox_words(seed, n, g)] == [int(v) for v in exp]
    # find misses among 4000 draws x 256 rows (~2 expected) and check them against the normals of the oracle
    d, N = 256, 4000
    W = sr.philox_words(seed, np.arange(N, dtype=np.uint64)[:, None], np.arange(d // 4, dtype=np.uint64)[None, :])
    mag = (W & np.uint64(0x7FFFFFFF)).transpose(1, 2, 0).reshape(N, d)
    hits = np.argwhere(mag < sr.MISS_BELOW)
    assert sr.miss_count(seed, d, np.arange(N)) == len(hits) >= 1
    for n, row in hits:
        u = po.randn_fill(seed, d, 1, int(n))[row, 0]
        x2 = sr.philox_words(seed, int(n), row // 4, word3=1)[row % 4]
        x = W[row % 4, n, row // 4]
        assert u == po.icdf_words([int(x)], [int(x2)])[0] and abs(u) > 4.5
