"""GPU parity of the fit: history walk (`gilbert_init`, curvature test, ring buffer; reference src/inverse_hessian.jl:5-66), Byrd compact form
(:98-133), `pdfactorize` / logdet / mean (src/woodbury.jl:201-207, src/mvnormal.jl:14-21) in every kernel (register-resident, TSQR, panel,
memory-resident; lean / prefetching / memory-resident walks), the Woodbury operator surface (src/woodbury.jl:129-165, 326-423), and the device
L-BFGS that produces traces -- against the CPU oracle, the reference's S0/Y0 fixture and dense algebra, through the C ABI."""
from concurrent.futures import ThreadPoolExecutor
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

from helpers import demo_device_target, fit_seeds, make_traces, oracle_factor_from_gpu, oracle_target
from oracle import pf_oracle as po
import margins as mg
from gpu_common import CASES, MIN_STRICT, _oracle_factor, _qr_ratio, _setup, _well_conditioned

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,K,J", CASES)
def test_fit_batch_matches_oracle(pfmi_mod, eng, name, K, J):
    """fit_mvnormals / lbfgs_inverse_hessians / pdfactorize (src/mvnormal.jl:14-21, src/inverse_hessian.jl:25-133,
    src/woodbury.jl:201-207): status, effective history, rejected updates, logdet, mu, and the dense
    W = A + B D B' rebuilt from the GPU factors."""
    tg, traces = _setup(pfmi_mod, eng, name, K, J)
    status, jeff, logdet, nrej = eng.fit_status()
    otg = oracle_target(tg)
    cfg = f"small:{name}"
    n_strict = n_wide = 0
    for k, tr in enumerate(traces):
        p0 = int(eng.offsets[k])
        P = len(tr)
        ref = po.path_fit_elbo(tr.points, tr.gradients, J, otg, 0, np.zeros(P, dtype=np.uint64))
        np.testing.assert_array_equal(status[p0:p0 + P], ref["status"])
        np.testing.assert_array_equal(jeff[p0:p0 + P], ref["j_eff"])
        assert nrej[k] == ref["n_rejected"]
        ok = ref["status"] == 0
        mg.check(cfg, "logdet", mg.rel(logdet[p0:p0 + P][ok], ref["logdet"][ok]))
        mg.record(cfg, "logdet_abs", np.abs(logdet[p0:p0 + P][ok] - ref["logdet"][ok]), np.inf)
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        for l in sorted(set(list(range(min(P, 9))) + [P // 2, min(P - 1, 2 * J + 3), P - 1])):
            if not ok[l]:
                continue
            f = eng.get_fit(p0 + l, int(jeff[p0 + l]))
            n_wide += int(2 * int(jeff[p0 + l]) > tg.d)
            mu_ref = ref["mu"][l]
            mg.check(cfg, "mu", np.max(np.abs(f["mu"] - mu_ref)) / (1 + np.abs(mu_ref).max()))
            np.testing.assert_allclose(f["alpha"], alpha_all[l], rtol=1e-12)
            j = int(hl[l])
            S = np.stack([tr.points[s + 1] - tr.points[s] for s in hs[l, :j]], axis=1) if j else np.zeros((tg.d, 0))
            Y = np.stack([tr.gradients[s] - tr.gradients[s + 1] for s in hs[l, :j]], axis=1) if j else np.zeros((tg.d, 0))
            B, D = po.lbfgs_inverse_hessian(alpha_all[l], S, Y)
            Wref = np.diag(alpha_all[l]) + B @ D @ B.T
            Wgpu = np.diag(f["alpha"]) + f["B"] @ f["D"] @ f["B"].T
            # SURVEY 8(d) as written: max |dW| <= 1e-11 max |W|, no conditioning allowance (until round 4 the
            # deviation was divided by cond(D)^(1/2) before the comparison; the recorded margins never needed it)
            mg.check(cfg, "W", np.max(np.abs(Wgpu - Wref)) / np.abs(Wref).max())
            assert f["B"].shape == (tg.d, 2 * j)                       # size(Σ.B) == (d, 2j), test/singlepath.jl:41
            # the factor itself: R = [V 0;0 I] Q' U,  W = R'R   (src/woodbury.jl:178-187)
            F = po.Factor(alpha_all[l], B, D)
            kk = min(tg.d, 2 * j)
            if kk:
                # (a) self-consistency of the GPU factor: R = [V 0;0 I] Q' U rebuilt from (U, Vh, T, V) gives W = R'R
                Vh = np.tril(f["qr_factors"][:, :kk], -1) + np.eye(tg.d, kk)
                Q = np.eye(tg.d) - Vh @ f["T"] @ Vh.T
                np.testing.assert_allclose(Q.T @ Q, np.eye(tg.d), atol=1e-12)
                blk = np.eye(tg.d); blk[:kk, :kk] = f["V"]
                Rm = blk @ Q.T @ np.diag(np.sqrt(f["alpha"]))
                assert np.max(np.abs(Rm.T @ Rm - Wref)) <= 1e-10 * np.abs(Wref).max() * max(1.0, np.linalg.cond(D) ** 0.5)
                assert abs(f["logdet"] - np.linalg.slogdet(Wref)[1]) <= 1e-8 * (1 + abs(f["logdet"]))
                # (b) reflector-level parity with the oracle (LAPACK convention) whenever the QR is well
                #     conditioned; for rank-deficient B~ (e.g. iso: y == s) later reflectors are roundoff-defined
                if _well_conditioned(F):
                    n_strict += 1
                    amp = 1e-13 / _qr_ratio(F)            # roundoff amplification of the reflectors
                    np.testing.assert_allclose(f["V"], F.V[:kk, :kk], rtol=1e-8, atol=max(1e-9, amp) * np.abs(F.V).max())
                    np.testing.assert_allclose(f["qr_factors"], F.QR[:, :2 * j], rtol=1e-8,
                                               atol=max(1e-9, amp) * np.abs(F.QR).max())
                    z = np.eye(tg.d, order="F").copy(order="F")
                    po.lib().pfo_apply_q(tg.d, kk, po._p(F.QR), po._p(F.tau), 0, po._p(z), tg.d)
                    np.testing.assert_allclose(Q, z, atol=max(1e-10, amp))
    assert n_strict >= MIN_STRICT.get(name, 3 * K), (name, n_strict)
    if name == "lr10":
        assert n_wide >= 3 * K, n_wide                     # fits with 2j > d really ran (k = d, R is d x 2j upper trapezoidal)


def test_reference_fixture_S0Y0_through_gpu(pfmi_mod, eng, golden_dir):
    """reference test/inverse_hessian.jl:19-44 on the GPU: the literal S0/Y0 history (as a trace whose
    steps are the fixture columns) reproduces the explicit dense Byrd formula, incl. ring rotation."""
    g = json.load(open(os.path.join(golden_dir, "lbfgs_S0Y0.json")))
    S = np.array(g["S0_columns"]).T
    Y = np.array(g["Y0_columns"]).T
    n, nh = S.shape
    theta = np.zeros((nh + 1, n)); grad = np.zeros((nh + 1, n))
    for l in range(nh):
        theta[l + 1] = theta[l] + S[:, l]
        grad[l + 1] = grad[l] - Y[:, l]
    for J in (3, 5):
        eng.set_traces([theta], [grad])
        eng.fit_batch(J)
        status, jeff, _, nrej = eng.fit_status()
        assert nrej[0] == 0 and list(jeff) == [min(l, J) for l in range(nh + 1)]
        for l in range(nh + 1):
            f = eng.get_fit(l, int(jeff[l]))
            j = int(jeff[l])
            if j == 0:
                np.testing.assert_allclose(f["alpha"], 1.0)
                continue
            Sl, Yl = S[:, l - j:l], Y[:, l - j:l]
            H0 = np.diag(f["alpha"])
            R = np.triu(Sl.T @ Yl); Rinv = np.linalg.inv(R)
            Bx = np.hstack([H0 @ Yl, Sl])
            Dx = np.block([[np.zeros((j, j)), -Rinv], [-Rinv.T, Rinv.T @ (np.diag(np.diag(R)) + Yl.T @ H0 @ Yl) @ Rinv]])
            Hexp = H0 + Bx @ Dx @ Bx.T
            Hgpu = H0 + f["B"] @ f["D"] @ f["B"].T
            np.testing.assert_allclose(Hgpu, Hexp, rtol=1e-9, atol=1e-10 * np.abs(Hexp).max())


def test_isonormal_exact_after_one_iteration_on_gpu(pfmi_mod, eng):
    """reference test/singlepath.jl:13-41 (BASELINE config 1 numerics): mu ~ 0, Sigma ~ I, size(B) = (d, 2)."""
    rng = np.random.default_rng(1)
    for d in (1, 5, 10, 100):
        th0 = rng.normal(size=d)
        eng.set_target(pfmi_mod.t_iso(d))
        eng.set_traces([np.stack([th0, np.zeros(d)])], [np.stack([-th0, np.zeros(d)])])
        eng.fit_batch(6)
        f = eng.get_fit(1, 1)
        assert f["B"].shape == (d, 2)
        np.testing.assert_allclose(f["mu"], 0, atol=1e-6)
        np.testing.assert_allclose(np.diag(f["alpha"]) + f["B"] @ f["D"] @ f["B"].T, np.eye(d), atol=1e-6)
        elbo, se, best = eng.elbo_batch(100, np.array([1, 2], dtype=np.uint64))
        assert best[0] == 1 and abs(elbo[1] - d / 2 * np.log(2 * np.pi)) < 1e-9 * d + 1e-9


def test_not_pd_fit_reports_status_and_nan_elbo(pfmi_mod, eng):
    """src/woodbury.jl:202,205: a non-PD fit is a per-fit status + NaN ELBO, never an abort; other paths proceed."""
    d = 8
    tg = pfmi_mod.t_iso(d)
    good = make_traces(tg, 1, 3)[0]
    theta = np.array([np.ones(d), np.zeros(d), -np.ones(d) * 0.5])
    grad = -theta.copy(); grad[2] = grad[1] * 0 + 1e-3 * np.arange(1, d + 1)   # inconsistent curvature on step 2
    eng.set_target(tg)
    eng.set_traces([theta, good.points], [grad, good.gradients])
    eng.fit_batch(6)
    status, jeff, logdet, nrej = eng.fit_status()
    ref = po.path_fit_elbo(theta, grad, 6, oracle_target(tg), 0, np.zeros(3, dtype=np.uint64))
    np.testing.assert_array_equal(status[:3], ref["status"])
    assert nrej[0] == ref["n_rejected"]
    for N in (32, 200):                                    # two-pass kernel (N < 64) and single-pass scan (N >= 64)
        elbo, se, best = eng.elbo_batch(N, fit_seeds(eng.P, 2))
        assert np.all(np.isfinite(elbo[4:]))
        if np.any(status[:3] != 0):
            assert np.all(np.isnan(elbo[:3][status[:3] != 0]))
            lp, lq = eng.elbo_logs(int(np.flatnonzero(status[:3] != 0)[0]), N)
            assert np.all(np.isnan(lp)) and np.all(np.isnan(lq))
    if np.any(status[:3] != 0):
        with pytest.raises(pfmi_mod.PosDefException):
            pfmi_mod.fit_mvnormals(theta, grad, history_length=6, engine=eng)


@pytest.mark.parametrize("d,maxit", [(2500, 14), (10000, 8)])
def test_large_d_general_paths(pfmi_mod, eng, d, maxit):
    """d beyond the resident-LDS / register kernels (config-5 style: funnel, history_length = 10 -> KC = 20, d = 2500 and the
    full d = 10^4): the streamed single-pass ELBO scan (V_h through LDS in 256-row chunks, head transform across two blocks)
    and the memory-resident fit kernel against the oracle; draw-writing launches take the lane-per-draw kernel."""
    J = 10
    tg = pfmi_mod.t_funnel(d)
    rng = pfmi_mod.HostRNG(5)
    traces = [pfmi_mod.optimize_with_trace(tg, rng.rand(d) * 2 - 1, history_length=J, maxiters=maxit) for _ in range(2)]
    eng.set_target(tg)
    eng.set_traces([t.points for t in traces], [t.gradients for t in traces])
    eng.fit_batch(J)
    status, jeff, logdet, nrej = eng.fit_status()
    seeds = fit_seeds(eng.P, 8)
    N = 64
    elbo, se, best = eng.elbo_batch(N, seeds)
    otg = oracle_target(tg)
    for k, tr in enumerate(traces):
        p0, p1 = int(eng.offsets[k]), int(eng.offsets[k + 1])
        ref = po.path_fit_elbo(tr.points, tr.gradients, J, otg, N, seeds[p0:p1])
        np.testing.assert_array_equal(status[p0:p1], ref["status"])
        np.testing.assert_array_equal(jeff[p0:p1], ref["j_eff"])
        ok = ref["status"] == 0
        mg.check("c5-shape:funnel-2x25", "logdet", mg.rel(logdet[p0:p1][ok], ref["logdet"][ok]))
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        for l in range(1, p1 - p0):
            if not ok[l]:
                continue
            F = _oracle_factor(tr, alpha_all, hl, hs, l, d)
            if _well_conditioned(F):
                mg.check("c5-shape:funnel-2x25", "elbo", mg.rel(elbo[p0 + l], ref["elbo"][l]), ctx=(k, l))
            else:
                assert abs(elbo[p0 + l] - ref["elbo"][l]) <= 8 * max(se[p0 + l], ref["se"][l]) + 1e-8 * (1 + abs(ref["elbo"][l]))
    p = int(eng.offsets[0]) + 2
    X, lp, lq = eng.draws(p, seeds[p], 32)
    np.testing.assert_allclose(lp, tg.logp(X), rtol=1e-9, atol=1e-6)
    assert np.max(np.abs(eng.logpdf(p, X) - lq)) <= 1e-8 * (1 + np.abs(lq).max())


@pytest.mark.parametrize("name,K,J", [("iso10", 1, 6), ("lr50", 2, 6), ("diag30", 1, 10), ("lr10", 1, 8), ("lr10", 1, 6)])
def test_woodbury_operator_surface(pfmi_mod, eng, name, K, J):
    """remaining PDMats surface on the device vs dense algebra and the oracle's own factor (reference test/woodbury.jl:239-402): what ties
    the device's factor to W itself -- W*x / W\\x / quad / invquad / diag against F.dense(), matrices and vectors -- and L, R and their
    inverses against the oracle's independently computed factor where its QR is well conditioned; the lr10 cases are the n < m ones
    (d = 10, 2j = 16 / 12: test/woodbury.jl:21-31 has n = 5, m = 8).  The operators' own arithmetic -- every op under a derived bound
    against long double at every column padding, head-block edge and block edge, and the round trips L (L \\ x) = x, R \\ (R x) = x as
    long-double residuals with no conditioning gate -- is in tests/test_gpu_woodbury.py."""
    tg, traces = _setup(pfmi_mod, eng, name, K, J)
    status, jeff, logdet, _ = eng.fit_status()
    rng = np.random.default_rng(5)
    tr = traces[0]
    alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
    n_strict = n_wide = 0
    for l in sorted({0, 1, min(4, len(tr) - 1), min(len(tr) - 1, J + 2), min(len(tr) - 1, 2 * J + 1), len(tr) - 1}):
        if status[l] != 0:
            continue
        F = _oracle_factor(tr, alpha_all, hl, hs, l, tg.d)
        n_wide += int(2 * int(hl[l]) > tg.d)
        W = F.dense()
        X = rng.normal(size=(tg.d, 9))
        tol = dict(rtol=1e-8, atol=1e-9 * max(1.0, np.abs(W).max()))
        np.testing.assert_allclose(eng.woodbury_apply(l, "mul", X), W @ X, **tol)
        np.testing.assert_allclose(eng.woodbury_apply(l, "solve", X), np.linalg.solve(W, X), rtol=1e-6, atol=1e-7 * np.abs(np.linalg.solve(W, X)).max())
        np.testing.assert_allclose(eng.woodbury_apply(l, "quad", X), np.einsum("ij,ij->j", X, W @ X), rtol=1e-8)
        np.testing.assert_allclose(eng.woodbury_apply(l, "invquad", X), np.einsum("ij,ij->j", X, np.linalg.solve(W, X)), rtol=1e-6)
        np.testing.assert_allclose(eng.woodbury_diag(l), np.diag(W), rtol=1e-9, atol=1e-12)
        x = X[:, 0].copy()
        np.testing.assert_allclose(eng.woodbury_apply(l, "mul", x), W @ x, **tol)
        # L and R themselves agree with the oracle's factor when the QR is well conditioned
        if _well_conditioned(F):
            n_strict += 1
            np.testing.assert_allclose(eng.woodbury_apply(l, "unwhiten", X), F.lmul_L(X), rtol=1e-7, atol=1e-8 * np.abs(X).max() * np.sqrt(np.abs(W).max()))
            np.testing.assert_allclose(eng.woodbury_apply(l, "rmul", X), F.lmul_R(X), rtol=1e-7, atol=1e-8 * np.abs(X).max() * np.sqrt(np.abs(W).max()))
            np.testing.assert_allclose(eng.woodbury_apply(l, "whiten", X), F.ldiv_L(X), rtol=1e-6, atol=1e-7 * np.abs(F.ldiv_L(X)).max())
            np.testing.assert_allclose(eng.woodbury_apply(l, "invunwhiten", X), F.ldiv_R(X), rtol=1e-6, atol=1e-7 * np.abs(F.ldiv_R(X)).max())
    assert n_strict >= MIN_STRICT.get(name, 2), (name, n_strict)
    if name == "lr10":
        assert n_wide >= 2, n_wide


@pytest.mark.gpu
def test_woodbury_inv_and_scaling_build_host_objects(pfmi_mod):
    """inv(W) and W * c (reference src/woodbury.jl:317-321, 357-360, test/woodbury.jl inv / * testsets): new WoodburyPDMat objects built
    on the host from the downloaded factor -- inv(F) = (U'^-1, Q, V'^-1), (A, B, D) = pdunfactorize -- against dense algebra."""
    tg = pfmi_mod.t_lowrank(40, r=8, seed=5)
    res = pfmi_mod.pathfinder(tg, ndraws=10, rng=pfmi_mod.HostRNG(3), history_length=6, ndraws_elbo=20)
    n_checked = 0
    for dist_ in (res.fit_distributions[2], res.fit_distributions[len(res.fit_distributions) - 1], res.fit_distribution):
        W = dist_.Sigma
        Wd = W.dense()
        Wi = W.inv()
        assert Wi.B.shape == W.B.shape and Wi.D.shape == W.D.shape
        np.testing.assert_allclose(Wi.dense(), np.linalg.inv(Wd), rtol=1e-8, atol=1e-10 * np.abs(np.linalg.inv(Wd)).max())
        np.testing.assert_allclose(Wi.diag(), np.diag(np.linalg.inv(Wd)), rtol=1e-8)
        assert abs(Wi.logdet + W.logdet) < 1e-12 and abs(W.logdet - np.linalg.slogdet(Wd)[1]) < 1e-8 * (1 + abs(W.logdet))
        Q1 = W.thin_Q()
        np.testing.assert_allclose(Q1.T @ Q1, np.eye(Q1.shape[1]), atol=1e-12)
        W3 = W * 3.0
        np.testing.assert_allclose(W3.dense(), 3.0 * Wd, rtol=1e-12, atol=1e-13 * np.abs(Wd).max())
        assert abs(W3.logdet - np.linalg.slogdet(3.0 * Wd)[1]) < 1e-8 * (1 + abs(W3.logdet))
        np.testing.assert_allclose((2.0 * W).dense(), 2.0 * Wd, rtol=1e-12, atol=1e-13 * np.abs(Wd).max())
        np.testing.assert_allclose(W * -1.0, -Wd, rtol=1e-13)            # c <= 0: the dense matrix (src/woodbury.jl:358)
        with pytest.raises(RuntimeError):
            Wi.mul(np.ones(40))
        n_checked += 1
    assert n_checked == 3


def test_woodbury_remaining_surface_like_reference_testsets(pfmi_mod):
    """reference test/woodbury.jl:228-309 on a fitted covariance of a real run: adjoint / transpose, + UniformScaling, right division,
    PDMats.dim (the operators themselves: test_gpu_fit.py::test_woodbury_operator_surface)"""
    tg = pfmi_mod.t_lowrank(12, 3, 5)
    res = pfmi_mod.pathfinder(tg, init=np.linspace(-1.0, 1.0, 12), rng=pfmi_mod.HostRNG(3), ndraws=10)
    W = res.fit_distribution.Sigma
    Wm = W.dense()
    n = 12
    assert W.T is W and W.dim == n
    c = 0.37
    np.testing.assert_allclose(W + c, Wm + c * np.eye(n), rtol=1e-12)
    np.testing.assert_allclose(c + W, c * np.eye(n) + Wm, rtol=1e-12)
    rng = np.random.default_rng(2)
    x = rng.normal(size=n)
    np.testing.assert_allclose(W.rdiv(x), np.linalg.solve(Wm, x), rtol=1e-7, atol=1e-9)          # x' / W = (W \ x)'
    X = rng.normal(size=(2, n))
    np.testing.assert_allclose(W.rdiv(X), np.linalg.solve(Wm, X.T).T, rtol=1e-7, atol=1e-9)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tname,d,J", [("diag", 2100, 6), ("lr", 1500, 6), ("funnel", 2500, 10)])
def test_memory_resident_fit_kernel_at_large_d(pfmi_mod, eng, tname, d, J, monkeypatch):
    """the column-by-column memory-resident kernel (fused reflector-apply + next-column dots, two Gram rows per sweep; the large-d
    default of round 1, now behind PFMI_FIT_KERNEL=mem and for d > 16384): dense W / logdet / mu against the oracle at four fits
    of the first path."""
    monkeypatch.setenv("PFMI_FIT_KERNEL", "mem")
    tg = {"diag": lambda d: pfmi_mod.t_diag(d, 1), "lr": lambda d: pfmi_mod.t_lowrank(d, 8, 2), "funnel": pfmi_mod.t_funnel}[tname](d)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(3).rand(2 * d).reshape(2, d) * (20 if tname == "funnel" else 4) - (10 if tname == "funnel" else 2)
    eng.optimize_batch(x0, J, 25)
    eng.fit_batch(J)
    st, je, ld, nr = eng.fit_status()
    th, _, gr = eng.get_trace(0, logp=False)
    alpha_all, hl, hs, _ = po.lbfgs_history(th, gr, J)
    n_checked = 0
    for p in sorted({1, 2, len(th) // 2, len(th) - 1}):
        if st[p] != 0:
            continue
        fa = eng.get_fit(p, int(je[p]))
        F = _oracle_factor(type("T", (), {"points": th, "gradients": gr})(), alpha_all, hl, hs, p, d)
        assert int(je[p]) == int(hl[p])
        assert abs(F.logdet - fa["logdet"]) <= 1e-9 * (1 + abs(F.logdet))
        mu_o = F.fit_mean(th[p], gr[p])
        np.testing.assert_allclose(fa["mu"], mu_o, rtol=1e-7, atol=1e-8 * (1 + np.abs(mu_o).max()))
        Wa = np.diag(fa["alpha"]) + fa["B"] @ fa["D"] @ fa["B"].T if fa["B"].size else np.diag(fa["alpha"])
        Wo = F.dense()
        assert np.max(np.abs(Wa - Wo)) <= 1e-10 * np.abs(Wo).max() * max(1.0, np.linalg.cond(fa["D"]) ** 0.5 if fa["D"].size else 1.0)
        n_checked += 1
    assert n_checked >= 3


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tname,d,J,maxit", [("diag", 1500, 4, 12), ("lr", 3000, 6, 14), ("funnel", 6000, 10, 16), ("diag", 12000, 10, 14),
                                               ("diag", 2000, 16, 22), ("funnel", 10000, 10, 14), ("lr", 5000, 8, 14), ("diag", 16384, 5, 10), ("diag", 5000, 12, 26)])
def test_panel_fit_kernel_variants(pfmi_mod, eng, tname, d, J, maxit):
    """The large-d fit kernels (1024 < d <= 16384) in every instantiation.  Default since round 6: TSQR + Householder reconstruction
    (`fit_tsqr_kernel.hip`: row chunks factored in registers, the stack of their R factors, LAPACK's reflectors rebuilt from the LU of
    Q - S; KPAD 8, 12, 16, 20); the left-looking panel kernel of rounds 2 - 5 (`fit_panel_kernel.hip`: register panels of 4 / 2 columns,
    MFMA cross products; still the default at KPAD = 32) -- each case runs the default AND the other one (PFMI_FIT_KERNEL = panel / tsqr).
    Against the oracle: status, logdet, mu, reflector-level QR / T / V where the QR is well conditioned, W x through the factor; and
    against the column-by-column memory-resident kernel (PFMI_FIT_KERNEL=mem) on every fit."""
    tg = {"diag": lambda d: pfmi_mod.t_diag(d, 1), "lr": lambda d: pfmi_mod.t_lowrank(d, 8, 2), "funnel": pfmi_mod.t_funnel}[tname](d)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(4).rand(2 * d).reshape(2, d) * (20 if tname == "funnel" else 4) - (10 if tname == "funnel" else 2)
    eng.optimize_batch(x0, J, maxit)
    eng.fit_batch(J)
    st, je, ld, nr = eng.fit_status()
    fits = {p: eng.get_fit(p, int(je[p])) for p in range(eng.P)}
    old = os.environ.get("PFMI_FIT_KERNEL")
    other = "tsqr" if (2 * J > 20 and d < 4096) else "panel"  # the large-d kernel that is NOT the default at this shape
    try:
        os.environ["PFMI_FIT_KERNEL"] = "mem"
        eng.fit_batch(J)
        st2, je2, ld2, _ = eng.fit_status()
        fits2 = {p: eng.get_fit(p, int(je2[p])) for p in range(eng.P)}
        os.environ["PFMI_FIT_KERNEL"] = other
        eng.fit_batch(J)
        st3, je3, ld3, _ = eng.fit_status()
        fits3 = {p: eng.get_fit(p, int(je3[p])) for p in range(eng.P)}
    finally:
        if old is None:
            os.environ.pop("PFMI_FIT_KERNEL", None)
        else:
            os.environ["PFMI_FIT_KERNEL"] = old
    np.testing.assert_array_equal(st, st2)
    np.testing.assert_array_equal(je, je2)
    np.testing.assert_array_equal(st, st3)
    np.testing.assert_array_equal(je, je3)
    seen_m = set()
    n_strict = 0
    rng = np.random.default_rng(0)
    for k in range(2):
        th, _, gr = eng.get_trace(k, logp=False)
        p0 = int(eng.offsets[k])
        alpha_all, hl, hs, _ = po.lbfgs_history(th, gr, J)
        tr = type("T", (), {"points": th, "gradients": gr})()
        for l in range(len(th)):
            p = p0 + l
            if st[p] != 0:
                continue
            fa, fb = fits[p], fits2[p]
            j = int(je[p])
            seen_m.add(2 * j)
            assert abs(ld[p] - ld2[p]) <= 1e-9 * (1 + abs(ld2[p]))
            if l in (1, 2, 3, len(th) // 2, len(th) - 1):
                F = _oracle_factor(tr, alpha_all, hl, hs, l, d)
                assert j == int(hl[l]) and F.status == 0
                assert abs(F.logdet - fa["logdet"]) <= 1e-9 * (1 + abs(F.logdet))
                mu_o = F.fit_mean(th[l], gr[l])
                np.testing.assert_allclose(fa["mu"], mu_o, rtol=1e-7, atol=1e-8 * (1 + np.abs(mu_o).max()))
                np.testing.assert_allclose(fa["D"], F.D, rtol=1e-6, atol=1e-9 * np.abs(F.D).max())
                if j:
                    X = rng.normal(size=(d, 3))
                    Wx = fa["alpha"][:, None] * X + fa["B"] @ (fa["D"] @ (fa["B"].T @ X))
                    np.testing.assert_allclose(Wx, F.mul_W(X), rtol=1e-8, atol=1e-9 * np.abs(Wx).max())
                    Vh = np.tril(fa["qr_factors"], -1) + np.eye(d, 2 * j)
                    G = Vh.T @ Vh                                        # Q'Q = I  <=>  T^-1 + T^-T = Vh'Vh
                    assert np.all(np.diag(fa["T"]) > 0)
                    np.testing.assert_allclose(np.linalg.inv(fa["T"]) + np.linalg.inv(fa["T"]).T, G, rtol=1e-9, atol=1e-10 * np.abs(G).max())
                    if _well_conditioned(F):
                        n_strict += 1
                        amp = 1e-13 / _qr_ratio(F)
                        np.testing.assert_allclose(fa["V"], F.V[:2 * j, :2 * j], rtol=1e-8, atol=max(1e-9, amp) * np.abs(F.V).max())
                        np.testing.assert_allclose(fa["qr_factors"], F.QR[:, :2 * j], rtol=1e-8, atol=max(1e-9, amp) * np.abs(F.QR).max())
                        np.testing.assert_allclose(np.diag(fa["T"]), F.tau[:2 * j], rtol=1e-9, atol=1e-12)
            # both large-d kernels vs the column-by-column kernel: same reflectors up to the conditioning of the block
            scale = max(np.abs(fb["qr_factors"]).max(), 1e-300) if j else 1.0
            Rd = np.abs(np.diag(fb["qr_factors"][:2 * j, :2 * j])) if j else np.ones(1)
            amp = 1e-12 * (Rd.max() / max(Rd.min(), 1e-300)) if j else 0.0
            for fx, ldx in ((fa, ld[p]), (fits3[p], ld3[p])):
                assert abs(ldx - ld2[p]) <= 1e-9 * (1 + abs(ld2[p]))
                if j and amp < 1e-6:
                    np.testing.assert_allclose(fx["qr_factors"], fb["qr_factors"], rtol=1e-7, atol=max(1e-10, amp) * scale)
                    np.testing.assert_allclose(fx["T"], fb["T"], rtol=1e-7, atol=max(1e-10, amp))
                np.testing.assert_allclose(fx["mu"], fb["mu"], rtol=1e-7, atol=1e-8 * (1 + np.abs(fb["mu"]).max()))
                np.testing.assert_allclose(fx["D"], fb["D"], rtol=1e-6, atol=1e-9 * max(np.abs(fb["D"]).max(), 1e-300) if j else 0.0)
    assert n_strict >= 2, n_strict
    assert any(mm % 4 == 2 for mm in seen_m) and max(seen_m) == 2 * J, seen_m      # ragged last panel and the full history both ran


@pytest.mark.parametrize("name,K,J", [("iso10", 2, 6), ("lr50", 2, 6), ("diag30", 2, 10), ("funnel12", 2, 6)])
def test_memory_resident_fit_kernel_matches_oracle(pfmi_mod, eng, name, K, J):
    """the general fit kernel (the default only for d > 1024 or J > 8) forced onto the small oracle cases:
    same dense W / logdet / mu / reflector-level checks as test_fit_batch_matches_oracle."""
    old = os.environ.get("PFMI_FIT_KERNEL")
    os.environ["PFMI_FIT_KERNEL"] = "mem"
    try:
        test_fit_batch_matches_oracle(pfmi_mod, eng, name, K, J)
    finally:
        if old is None:
            os.environ.pop("PFMI_FIT_KERNEL", None)
        else:
            os.environ["PFMI_FIT_KERNEL"] = old


@pytest.mark.parametrize("tname,d,J", [("diag", 2500, 6), ("funnel", 6000, 10), ("diag", 10000, 10), ("diag", 8200, 4)])
def test_lean_history_walk_is_bit_identical_to_the_prefetching_one(pfmi_mod, tname, d, J, monkeypatch):
    """2048 < d <= 10 240: pf_history_lean_kernel (alpha + two row sets in registers, 1 / alpha in LDS) against pf_history_kernel
    (PFMI_HISTORY_KERNEL=prefetch): alpha of every point, effective history, ring sources, rejections -- and with them every fit --
    must be the same bits; both against the oracle's walk."""
    tg = pfmi_mod.t_funnel(d) if tname == "funnel" else pfmi_mod.t_diag(d, 1)
    sc = 10.0 if tname == "funnel" else 2.0
    K = 2
    x0 = pfmi_mod.HostRNG(17).rand(K * d).reshape(K, d) * 2 * sc - sc
    out = {}
    for mode in ("lean", "prefetch"):
        if mode == "prefetch":
            monkeypatch.setenv("PFMI_HISTORY_KERNEL", "prefetch")
        else:
            monkeypatch.delenv("PFMI_HISTORY_KERNEL", raising=False)
        e = pfmi_mod.Engine(0)
        try:
            e.set_target(tg)
            e.optimize_batch(x0, J, 30)
            e.fit_batch(J)
            st, je, ld, nr = e.fit_status()
            fits = [e.get_fit(p, int(je[p])) for p in sorted({1, e.P // 2, e.P - 1})]
            traces = [e.get_trace(k, logp=False) for k in range(K)]
            out[mode] = (st, je, nr, ld, [f["alpha"] for f in fits], [f["mu"] for f in fits], traces, e.offsets.copy())
        finally:
            e.close()
    a, b = out["lean"], out["prefetch"]
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a[4] + a[5], b[4] + b[5]):
        np.testing.assert_array_equal(x, y)
    for k, (th, _, gr) in enumerate(a[6]):
        alpha_all, hl, hs, nrej = po.lbfgs_history(th, gr, J)
        p0 = int(a[7][k])
        np.testing.assert_array_equal(a[1][p0:p0 + len(th)], hl)
        assert int(a[2][k]) == int(nrej)
    last = po.lbfgs_history(a[6][K - 1][0], a[6][K - 1][2], J)[0][-1]
    np.testing.assert_allclose(a[4][-1], last, rtol=1e-10)


@pytest.mark.parametrize("tname,d,J", [("diag", 700, 6), ("funnel", 3000, 10), ("diag", 12000, 4)])
def test_memory_resident_history_walk_matches_the_register_kernels(pfmi_mod, tname, d, J, monkeypatch):
    """PFMI_HISTORY_KERNEL=mem at sizes the register kernels own: the same accepted updates, ring sources and rejections; alpha to
    roundoff (the memory-resident walk divides like the reference, the register kernels carry 1 / alpha)."""
    tg = pfmi_mod.t_funnel(d) if tname == "funnel" else pfmi_mod.t_diag(d, 1)
    sc = 10.0 if tname == "funnel" else 2.0
    x0 = pfmi_mod.HostRNG(23).rand(2 * d).reshape(2, d) * 2 * sc - sc
    out = {}
    for mode in ("default", "mem"):
        if mode == "mem":
            monkeypatch.setenv("PFMI_HISTORY_KERNEL", "mem")
        else:
            monkeypatch.delenv("PFMI_HISTORY_KERNEL", raising=False)
        e = pfmi_mod.Engine(0)
        try:
            e.set_target(tg)
            e.optimize_batch(x0, J, 40)
            e.fit_batch(J)
            st, je, ld, nr = e.fit_status()
            pts = sorted({1, e.P // 2, e.P - 1})
            out[mode] = (st, je, nr, ld, [e.get_fit(p, int(je[p]))["alpha"] for p in pts])
        finally:
            e.close()
    a, b = out["default"], out["mem"]
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    okm = a[0] == 0
    mg.check(f"history mem d={d}", "logdet vs register walk", np.max(np.abs(a[3][okm] - b[3][okm]) / (1 + np.abs(a[3][okm]))), 1e-10)
    for x, y in zip(a[4], b[4]):
        mg.check(f"history mem d={d}", "alpha vs register walk", np.max(np.abs(x - y) / x), 1e-10)


# ---- device trajectory generation -----------------------------------------------------
@pytest.mark.parametrize("name,d,scale,maxit", [("iso", 10, 2, 1000), ("diag", 30, 2, 1000), ("lr", 50, 2, 1000), ("funnel", 12, 10, 60),
                                               ("lr", 1000, 2, 1000), ("diag", 3000, 2, 200), ("lr16", 600, 2, 1000), ("lr11", 200, 2, 1000),
                                               ("lr", 1500, 2, 300)])
def test_device_lbfgs_traces_match_oracle_driver(pfmi_mod, eng, name, d, scale, maxit):
    """pfmi_optimize_batch vs oracle pfo_optimize_trace (same algorithm, scalar C): early iterates agree to roundoff
    (later ones drift apart through line-search branches, as between any two L-BFGS implementations), every recorded
    (logp, grad) belongs to its recorded point, the objective never increases, Gaussian targets converge to g_tol.
    d = 1000 exercises the LDS ring, d = 3000 the global ring and the 512-thread variant; rank 16 / 11 the 16-column padding of the
    low-rank factor (its rows cached in registers), d = 1500 the low-rank target with rows re-read from memory."""
    tg = {"iso": pfmi_mod.t_iso, "diag": lambda d: pfmi_mod.t_diag(d, 1), "lr": lambda d: pfmi_mod.t_lowrank(d, 8, 2),
          "lr16": lambda d: pfmi_mod.t_lowrank(d, 16, 3), "lr11": lambda d: pfmi_mod.t_lowrank(d, 11, 4),
          "funnel": pfmi_mod.t_funnel}[name](d)
    ot = oracle_target(tg)
    K = 3
    x0 = pfmi_mod.HostRNG(3).rand(K * d).reshape(K, d) * 2 * scale - scale
    eng.set_target(tg)
    npts = eng.optimize_batch(x0, 6, maxit)
    assert np.all(npts >= 2) and np.all(npts <= maxit + 1)
    for k in range(K):
        th, lp, gr = eng.get_trace(k)
        assert th.shape == (npts[k], d) and np.array_equal(th[0], x0[k])
        P, L, G = po.optimize_trace(ot, x0[k], 6, maxit)
        n = min(len(P), len(th), 8)
        np.testing.assert_allclose(th[:n], P[:n], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(gr[:n], G[:n], rtol=1e-8, atol=1e-9 * max(1.0, np.abs(G[:n]).max()))
        for l in sorted({0, 1, len(th) // 2, len(th) - 1}):
            lpo, go = po.logp_grad(ot, th[l])
            assert abs(lpo - lp[l]) <= 1e-11 * max(1.0, abs(lpo))
            np.testing.assert_allclose(gr[l], go, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(go).max()))
        assert np.all(np.diff(lp) >= -1e-9 * np.maximum(1.0, np.abs(lp[1:])))
        if name != "funnel" and npts[k] <= maxit:
            assert np.abs(gr[-1]).max() <= 1e-8
            np.testing.assert_allclose(th[-1], P[-1], atol=1e-5)


def test_device_traces_feed_fit_batch_like_uploaded_ones(pfmi_mod, eng):
    """the traces pfmi_optimize_batch leaves in HBM are the same input pfmi_set_traces would upload: refitting from
    the downloaded copy gives bit-identical ELBOs."""
    tg = pfmi_mod.t_lowrank(64, 8, 2)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(7).rand(5 * 64).reshape(5, 64) * 4 - 2
    npts = eng.optimize_batch(x0, 6)
    seeds = fit_seeds(int(npts.sum()), 4)
    eng.fit_batch(6)
    e1, s1, b1 = eng.elbo_batch(200, seeds)
    traces = [eng.get_trace(k) for k in range(5)]
    eng.set_traces([t[0] for t in traces], [t[2] for t in traces])
    eng.fit_batch(6)
    e2, s2, b2 = eng.elbo_batch(200, seeds)
    np.testing.assert_array_equal(e1, e2)
    np.testing.assert_array_equal(b1, b2)
    with pytest.raises(pfmi_mod.PfmiError):
        eng.get_trace(0)                                   # log densities only exist for device-made traces
    eng.set_target(pfmi_mod.CallbackTarget(64, lambda x: 0.0))
    with pytest.raises(pfmi_mod.PfmiError):
        eng.optimize_batch(x0, 6)


# ---- device L-BFGS: the pair-rejected branch (second gather of S'g, Y'g over the unchanged ring) ---------------------------------
@pytest.mark.parametrize("name,d,J", [("lr", 200, 6), ("diag", 1500, 4), ("funnel", 40, 6)])
def test_device_lbfgs_rejected_pairs_follow_the_host_driver(pfmi_mod, name, d, J, monkeypatch):
    """A strong-Wolfe step always passes the curvature test, so the kernel's `pair rejected' branch (ring left as it is, inner
    products of the OLD ring with the new gradient gathered in a second pass) never runs on its own: PFMI_LBFGS_REJECT_EVERY=3 drops
    every third pair, pfmi/optimize.py (the host twin: two-loop recursion in NumPy) does the same, and the iterates must agree
    -- through several rejections, a full ring and its wrap-around."""
    from pfmi.optimize import optimize_with_trace
    tg = {"lr": lambda: pfmi_mod.t_lowrank(d, 8, 2), "diag": lambda: pfmi_mod.t_diag(d, 1), "funnel": lambda: pfmi_mod.t_funnel(d)}[name]()
    K = 3
    x0 = pfmi_mod.HostRNG(11).rand(K * d).reshape(K, d) * 4 - 2
    monkeypatch.setenv("PFMI_LBFGS_REJECT_EVERY", "3")
    e2 = pfmi_mod.Engine(0)
    try:
        e2.set_target(tg)
        npts = e2.optimize_batch(x0, J, 40)
        for k in range(K):
            th, lp, gr = e2.get_trace(k)
            ref = optimize_with_trace(tg, x0[k], J, 40, _reject_every=3)
            n = min(len(th), len(ref), 14)
            assert n >= 10, (n, npts)
            rt = 1e-5 if name == "funnel" else 1e-7           # (the funnel amplifies roundoff between the two recursions faster)
            np.testing.assert_allclose(th[:n], ref.points[:n], rtol=rt, atol=rt / 10)
            np.testing.assert_allclose(gr[:n], ref.gradients[:n], rtol=10 * rt, atol=rt * max(1.0, np.abs(ref.gradients[:n]).max()))
            assert np.all(np.diff(lp) >= -1e-9 * np.maximum(1.0, np.abs(lp[1:])))
    finally:
        e2.close()
    monkeypatch.delenv("PFMI_LBFGS_REJECT_EVERY")
    e3 = pfmi_mod.Engine(0)
    try:                                                     # and without the hook the host twin follows the kernel as well
        e3.set_target(tg)
        e3.optimize_batch(x0, J, 40)
        th, lp, gr = e3.get_trace(0)
        ref = optimize_with_trace(tg, x0[0], J, 40)
        n = min(len(th), len(ref), 14)
        np.testing.assert_allclose(th[:n], ref.points[:n], rtol=rt, atol=rt / 10)
    finally:
        e3.close()


@pytest.mark.parametrize("name,d,J,maxit", [("lr", 40, 1, 60), ("diag", 300, 2, 80), ("lr", 700, 10, 200), ("diag", 90, 16, 200), ("funnel", 20, 16, 60),
                                            ("lr", 2000, 16, 60), ("diag", 2500, 1, 40)])
def test_device_lbfgs_history_lengths_1_to_16(pfmi_mod, name, d, J, maxit):
    """the fused reduction of the device L-BFGS handles the ring in batches of 6 (d <= 1024) or 2 (d > 1024) pairs: history lengths
    that are one batch, several batches and a ragged last batch, a ring of one pair (every update evicts), on every workgroup shape --
    against the oracle driver (first iterates to roundoff) and by its own invariants (monotone, converged, recorded values consistent)."""
    tg = {"lr": lambda: pfmi_mod.t_lowrank(d, 8, 2), "diag": lambda: pfmi_mod.t_diag(d, 1), "funnel": lambda: pfmi_mod.t_funnel(d)}[name]()
    ot = oracle_target(tg)
    K = 2
    sc = 10.0 if name == "funnel" else 2.0
    x0 = pfmi_mod.HostRNG(13).rand(K * d).reshape(K, d) * 2 * sc - sc
    e = pfmi_mod.Engine(0)
    try:
        e.set_target(tg)
        npts = e.optimize_batch(x0, J, maxit)
        assert np.all(npts >= 2)
        for k in range(K):
            th, lp, gr = e.get_trace(k)
            P, L, G = po.optimize_trace(ot, x0[k], J, maxit)
            n = min(len(P), len(th), 10)
            rt = 1e-6 if name == "funnel" else 1e-8
            np.testing.assert_allclose(th[:n], P[:n], rtol=rt, atol=rt)
            for l in sorted({0, len(th) // 2, len(th) - 1}):
                lpo, go = po.logp_grad(ot, th[l])
                assert abs(lpo - lp[l]) <= 1e-10 * max(1.0, abs(lpo))
                np.testing.assert_allclose(gr[l], go, rtol=1e-9, atol=1e-10 * max(1.0, np.abs(go).max()))
            assert np.all(np.diff(lp) >= -1e-9 * np.maximum(1.0, np.abs(lp[1:])))
            if name != "funnel" and npts[k] <= maxit:
                assert np.abs(gr[-1]).max() <= 1e-8
    finally:
        e.close()
