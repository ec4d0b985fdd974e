"""GPU parity of the ELBO stage: `elbo_and_samples` / `maximize_elbo` / `_findmax_skipnan` (reference src/elbo.jl:1-20, src/utils.jl:55-72): ELBO / SE /
argmax against the oracle and analytic known answers, the single-pass scan against the lane kernel, bitwise independence of the launch geometry,
the in-kernel hand-over of the scan's last round, enqueue / wait twins, profiling modes, host and device closures as targets."""
from concurrent.futures import ThreadPoolExecutor
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest

from helpers import demo_device_target, fit_seeds, make_traces, oracle_factor_from_gpu, oracle_target
from oracle import pf_oracle as po
import margins as mg
from gpu_common import CASES, MIN_STRICT, _oracle_factor, _setup, _well_conditioned

pytestmark = pytest.mark.gpu


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


PROBE = os.path.join(ROOT, "tests", "probes", "handover_stress.py")


def _run(cmd, timeout):
    env = dict(os.environ, PFMI_DEBUG_HOOKS="1", TMPDIR="/tmp")
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout)
    return r.returncode, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("name,K,J", CASES)
def test_elbo_batch_matches_oracle(pfmi_mod, eng, name, K, J):
    """maximize_elbo (src/elbo.jl:1-20) over every path: ELBO, SE, NaN-skipping argmax."""
    tg, traces = _setup(pfmi_mod, eng, name, K, J)
    otg = oracle_target(tg)
    N = 200
    seeds = fit_seeds(eng.P, 5)
    elbo, se, best = eng.elbo_batch(N, seeds)
    # parity mode with uploaded normals gives the same answers as the in-kernel generator
    U = np.concatenate([po.randn_fill(int(seeds[p]), tg.d, N).T.ravel() for p in range(eng.P)])
    elbo_m, se_m, best_m = eng.elbo_batch(N, seeds, u=U)
    n_strict = 0
    for k, tr in enumerate(traces):
        p0, p1 = int(eng.offsets[k]), int(eng.offsets[k + 1])
        ref = po.path_fit_elbo(tr.points, tr.gradients, J, otg, N, seeds[p0:p1])
        assert np.isnan(elbo[p0]) and np.isnan(se[p0])
        alpha_all, hl, hs, _ = po.lbfgs_history(tr.points, tr.gradients, J)
        wc = np.array([ref["status"][l] == 0 and _well_conditioned(_oracle_factor(tr, alpha_all, hl, hs, l, tg.d))
                       for l in range(1, p1 - p0)])
        for a, b, sa, sb in ((elbo, ref["elbo"], se, ref["se"]), (elbo_m, ref["elbo"], se_m, ref["se"])):
            x, y = a[p0 + 1:p1], b[1:]
            fin = np.isfinite(y)
            np.testing.assert_array_equal(np.isfinite(x), fin)
            strict = fin & wc
            n_strict += int(strict.sum())
            mg.check(f"small:{name}", "elbo", mg.rel(x[strict], y[strict]))
            mg.check(f"small:{name}", "se", mg.rel(sa[p0 + 1:p1][strict], sb[1:][strict]))
            loose = fin & ~wc     # rank-deficient QR: same distribution, roundoff-defined draws -> statistical agreement
            tol = 8 * np.maximum(sa[p0 + 1:p1][loose], sb[1:][loose]) + 1e-9 * (1 + np.abs(y[loose]))
            assert np.all(np.abs(x[loose] - y[loose]) <= tol)
        vals = ref["elbo"][1:]
        top = np.sort(vals[np.isfinite(vals)])[-2:] if np.sum(np.isfinite(vals)) >= 2 else None
        if np.all(wc) and (top is None or top[1] - top[0] > 1e-8 * (1 + abs(top[1]))):
            assert best[k] == ref["best_iter"] == best_m[k]
        lp, lq = eng.elbo_logs(p0 + int(best[k]), N)
        v, s, _ = po.elbo_stats(lp, lq)
        assert abs(v - elbo[p0 + int(best[k])]) <= 1e-10 * (1 + abs(v))
        # per-draw log densities of the production launch against the oracle's own draws of the same fit
        if wc[int(best[k]) - 1] and best[k] == ref["best_iter"]:
            refd = po.path_fit_elbo(tr.points, tr.gradients, J, otg, N, seeds[p0:p1], want_draws=True)
            mg.check(f"small:{name}", "logp@scan", mg.rel(lp, refd["logp"]))
            mg.check(f"small:{name}", "logq@scan", mg.rel(lq, refd["logq"]))
    assert n_strict >= MIN_STRICT.get(name, 8 * K), (name, n_strict)


@pytest.mark.parametrize("sigma", [1e-3, 0.05, 0.8, 1.0, 1.1, 1.2, 5.0, 10.0])
def test_analytic_elbo_known_answer_on_gpu(pfmi_mod, eng, sigma):
    """reference test/elbo.jl:7-28 on the GPU: 1-D, ELBO = (1 - r^2)/2 + log r within 3 SE.  A 1-D Normal(0, sigma)
    is obtained as the fit of a one-step trace on the quadratic with curvature 1/sigma^2."""
    sigma_t = 0.08
    tgt = pfmi_mod.GaussTarget(np.zeros(1), np.array([sigma_t**2]), offset=-0.5 * np.log(2 * np.pi) - np.log(sigma_t))
    th0 = 0.3
    theta = np.array([[th0], [0.0]])
    grad = np.array([[-th0 / sigma**2], [0.0]])      # gradient of -x^2/(2 sigma^2): one exact Newton step
    eng.set_target(tgt)
    eng.set_traces([theta], [grad])
    eng.fit_batch(6)
    f = eng.get_fit(1, 1)
    Sig = f["alpha"][0] + (f["B"] @ f["D"] @ f["B"].T)[0, 0]
    assert abs(Sig - sigma**2) < 1e-9 * sigma**2 and abs(f["mu"][0]) < 1e-12
    N = 400_000
    elbo, se, best = eng.elbo_batch(N, np.array([0, 4242], dtype=np.uint64))
    r = sigma / sigma_t
    assert abs(elbo[1] - ((1 - r * r) / 2 + np.log(r))) <= 3 * se[1] + 1e-12
    assert best[0] == 1


@pytest.mark.parametrize("tname,d,K,J,N,scale,maxit", [
    ("iso", 10, 2, 6, 100, 2, 1000), ("diag", 30, 2, 6, 200, 2, 1000), ("lr", 50, 2, 6, 200, 2, 1000), ("lr", 300, 2, 6, 500, 2, 1000),
    ("funnel", 12, 2, 6, 100, 10, 40), ("diag", 30, 2, 10, 200, 2, 1000), ("lr", 50, 2, 16, 200, 2, 1000),
    ("diag", 3000, 2, 6, 200, 2, 30), ("funnel", 2500, 2, 10, 300, 10, 30), ("lr", 1100, 2, 8, 130, 2, 40),
    ("lr", 64, 8, 6, 1000, 2, 45), ("diag", 48, 7, 4, 500, 2, 50),
    # KC = 16 / 20 at N >= 768, resident and streamed, every target family, ragged tails.  With K = 2 paths these are fewer than the 128
    # fits launch_qf wants for two groups per wave at KC >= 16, so they run ONE group per wave; the two-group instances <16 | 20, ., ., 2>
    # are compared with the extended-precision reference in test_gpu_scan_reference.py, which asserts the plan every scan ran
    ("funnel", 2000, 2, 10, 800, 10, 24), ("lr", 600, 2, 8, 1000, 2, 30), ("diag", 100, 2, 10, 784, 2, 40), ("lr", 1500, 2, 10, 770, 2, 24),
    ("lr", 3000, 2, 16, 200, 2, 20)])
def test_single_pass_scan_matches_lane_kernel(pfmi_mod, eng, tname, d, K, J, N, scale, maxit):
    """the single-pass quadratic-form scan (elbo_qf_kernel.hip: logp from per-draw contractions, x never formed; Vh resident or
    streamed through LDS; KC up to 32) against the lane-per-draw kernel that evaluates logp(x) on the materialised draw, same
    seeds: per-draw logp / logq and the per-fit ELBO agree to fp64 roundoff.  Covers the head transform spilling into
    block 1 (J = 10, 16), chunked streaming (d = 2500, 3000), ragged last block / last group and the low-rank target; the two
    K = 8 / 7 cases have more fits than the GPU has CUs and not a multiple of them, so the fits of the last partial round take the
    second, one-batch-per-workgroup launch (two groups per wave at N = 1000, one at N = 500)."""
    tg = {"iso": pfmi_mod.t_iso, "diag": lambda d: pfmi_mod.t_diag(d, 1), "lr": lambda d: pfmi_mod.t_lowrank(d, 8, 2),
          "funnel": pfmi_mod.t_funnel}[tname](d)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(3).rand(K * d).reshape(K, d) * 2 * scale - scale
    eng.optimize_batch(x0, J, maxit)
    eng.fit_batch(J)
    if K >= 7:
        nfits = eng.P - K
        assert nfits > 256 and nfits % 256 != 0, nfits               # the tail launch really runs
    seeds = fit_seeds(eng.P, 1)
    out = {}
    old = os.environ.get("PFMI_ELBO_KERNEL")
    try:
        for mode in ("lane", "qf"):
            os.environ["PFMI_ELBO_KERNEL"] = mode
            elbo, se, best = eng.elbo_batch(N, seeds)
            pts = sorted({1, min(3, eng.P - 1), eng.P // 2, eng.P - 1, max(eng.P - 7, 1), max(eng.P - 20, 1)})
            out[mode] = (elbo, se, best, [eng.elbo_logs(p, N) for p in pts])
    finally:
        if old is None:
            os.environ.pop("PFMI_ELBO_KERNEL", None)
        else:
            os.environ["PFMI_ELBO_KERNEL"] = old
    a, b = out["qf"], out["lane"]
    assert np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
    ok = np.isfinite(b[0])
    assert np.max(np.abs(a[0][ok] - b[0][ok]) / (1 + np.abs(b[0][ok]))) <= 1e-10
    oks = ok & np.isfinite(b[1])
    assert np.array_equal(np.isfinite(a[1][ok]), np.isfinite(b[1][ok]))
    assert np.max(np.abs(a[1][oks] - b[1][oks]) / (1 + np.abs(b[1][oks]))) <= 1e-8
    for (lpa, lqa), (lpb, lqb) in zip(a[3], b[3]):
        assert np.max(np.abs(lpa - lpb) / (1 + np.abs(lpb))) <= 1e-10
        assert np.max(np.abs(lqa - lqb) / (1 + np.abs(lqb))) <= 1e-12


# ---- failure handling on the GPU ---------------------------------------------------------------------------
def test_failed_fits_nan_elbos_and_skipnan_argmax_on_gpu(pfmi_mod, eng):
    """The chain non-PD fit -> per-fit status -> NaN ELBO -> NaN-skipping argmax, executed on the GPU and compared with the
    oracle.  A BFGS-accepted trace is PD in exact arithmetic, so the failures are injected:
      path 0  random (theta, grad) walk with the curvature threshold eps = -1e300 (the reference's `ϵ` keyword,
              src/inverse_hessian.jl:25): negative-curvature pairs are accepted -> alpha < 0 (A not PD, :202) and
              indefinite C = I + R D R' (:205);
      path 1  NaN gradient at the FIRST fitted point  -> NaN mean -> NaN ELBO first      (test/utils.jl:10)
      path 2  NaN gradient in the MIDDLE of the trace -> NaN ELBO in the middle           (test/utils.jl:9)
      path 3  NaN gradient everywhere                 -> all NaN -> (NaN, 1)              (test/utils.jl:11)
      path 4  clean trace."""
    d, J, eps = 8, 6, -1e300
    tg = pfmi_mod.t_diag(d, seed=3)
    otg = oracle_target(tg)
    rng = np.random.default_rng(0)
    bad_th = np.cumsum(rng.normal(size=(9, d)), 0)
    bad_gr = rng.normal(size=(9, d))
    good = make_traces(tg, 4, 3)
    ths = [bad_th] + [t.points.copy() for t in good]
    grs = [bad_gr] + [t.gradients.copy() for t in good]
    grs[1][1, 2] = np.nan
    grs[2][len(grs[2]) // 2, 0] = np.nan
    grs[3][:, 1] = np.nan
    eng.set_target(tg)
    eng.set_traces(ths, grs)
    eng.fit_batch(J, eps)
    status, jeff, logdet, nrej = eng.fit_status()
    refs = []
    for k in range(5):
        p0, p1 = int(eng.offsets[k]), int(eng.offsets[k + 1])
        ref = po.path_fit_elbo(ths[k], grs[k], J, otg, 0, np.zeros(p1 - p0, dtype=np.uint64), eps=eps)
        np.testing.assert_array_equal(status[p0:p1], ref["status"])
        np.testing.assert_array_equal(jeff[p0:p1], ref["j_eff"])
        assert nrej[k] == ref["n_rejected"]
        assert np.all(np.isnan(logdet[p0:p1][ref["status"] != 0]))
    p0 = int(eng.offsets[0])
    st0 = status[p0:int(eng.offsets[1])]
    assert set(st0.tolist()) >= {0, 1, 2}, st0                  # both PosDefException sites really fired on the GPU
    assert np.all(status[int(eng.offsets[1]):] == 0)            # a NaN gradient is rejected by the curvature test: the factor stays PD
    seeds = fit_seeds(eng.P, 2)
    for N, kern in ((32, None), (200, None), (200, "lane"), (200, "mfma")):      # two-pass (N < 64), single-pass scan, the others
        old = os.environ.get("PFMI_ELBO_KERNEL")
        if kern:
            os.environ["PFMI_ELBO_KERNEL"] = kern
        try:
            elbo, se, best = eng.elbo_batch(N, seeds)
        finally:
            if kern:
                os.environ.pop("PFMI_ELBO_KERNEL", None)
                if old is not None:
                    os.environ["PFMI_ELBO_KERNEL"] = old
        for k in range(5):
            p0, p1 = int(eng.offsets[k]), int(eng.offsets[k + 1])
            ref = po.path_fit_elbo(ths[k], grs[k], J, otg, N, seeds[p0:p1], eps=eps)
            np.testing.assert_array_equal(np.isnan(elbo[p0:p1]), np.isnan(ref["elbo"]))
            fin = np.isfinite(ref["elbo"])
            if k != 0:                                          # path 0 is indefinite garbage: only the NaN pattern / argmax logic
                assert np.all(np.abs(elbo[p0:p1][fin] - ref["elbo"][fin]) <= 1e-9 * (1 + np.abs(ref["elbo"][fin])))
                assert best[k] == ref["best_iter"], (N, kern, k)
            else:                                               # argmax of the GPU's own values with the reference's rule
                assert best[k] == po.findmax_skipnan(elbo[p0 + 1:p1])[1]
            failed = np.flatnonzero(status[p0:p1] != 0)
            assert np.all(np.isnan(elbo[p0:p1][failed])) and np.all(np.isnan(se[p0:p1][failed]))
            for l in failed[:2]:
                lp, lq = eng.elbo_logs(p0 + int(l), N)
                assert np.all(np.isnan(lp)) and np.all(np.isnan(lq))
        # the three NaN placements of test/utils.jl:8-12
        p1_ = int(eng.offsets[1])
        assert np.isnan(elbo[p1_ + 1]) and best[1] > 1                       # NaN first: a later finite value wins
        mid = len(grs[2]) // 2
        p2_ = int(eng.offsets[2])
        assert np.isnan(elbo[p2_ + mid]) and best[2] != mid and np.isfinite(elbo[p2_ + best[2]])
        p3_ = int(eng.offsets[3])
        assert np.all(np.isnan(elbo[p3_:int(eng.offsets[4])])) and best[3] == 1   # all NaN -> (NaN, 1)
    # WoodburyPDMat's constructor throws (src/woodbury.jl:202,205): fit_mvnormals mirrors it
    with pytest.raises(pfmi_mod.PosDefException):
        pfmi_mod.fit_mvnormals(bad_th, bad_gr, history_length=J, engine=eng, eps=eps)
    dists, nrej1 = pfmi_mod.fit_mvnormals(good[0].points, good[0].gradients, history_length=J, engine=eng)
    assert len(dists) == len(good[0]) and nrej1 == 0


# ---- results do not depend on the launch geometry (found by the G > 1 runs of round 3) --------------------------------------
@pytest.mark.parametrize("N", [600, 1000])
def test_scan_is_bitwise_independent_of_launch_geometry(pfmi_mod, eng, N):
    """The ELBO scan cuts its work in launch-dependent ways: the fits beyond the last full round of CUs go into a tail launch of
    one-batch pieces, and a wave owns one or two 16-draw groups.  A fit's per-draw log densities -- hence its ELBO, hence
    best_iter -- must be the SAME BITS whichever way it was cut (the reference's `ntasks` invariance, test/multipath.jl:107-140;
    here it also makes the result independent of the number of GPUs the paths are sharded over)."""
    d, J, K = 100, 6, 10
    tg = pfmi_mod.t_lowrank(d, r=8, seed=2)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(31).rand(K * d).reshape(K, d) * 4 - 2
    npts = eng.optimize_batch(x0, J)
    eng.fit_batch(J)
    nfits = eng.P - K
    assert nfits > 256 and nfits % 256 != 0, nfits              # a main launch AND a tail launch
    seeds = fit_seeds(eng.P, 12)
    elbo_a, se_a, best_a = eng.elbo_batch(N, seeds)
    last = eng.P - 1                                            # a fit of the tail launch
    logs_a = eng.elbo_logs(last, N)
    os.environ["PFMI_QF_NO_TAIL"] = "1"
    try:
        elbo_b, se_b, best_b = eng.elbo_batch(N, seeds)
        logs_b = eng.elbo_logs(last, N)
    finally:
        os.environ.pop("PFMI_QF_NO_TAIL", None)
    np.testing.assert_array_equal(logs_a[0], logs_b[0])
    np.testing.assert_array_equal(logs_a[1], logs_b[1])
    np.testing.assert_array_equal(elbo_a, elbo_b)
    np.testing.assert_array_equal(se_a, se_b)
    np.testing.assert_array_equal(best_a, best_b)
    # the pieces ride behind the whole fits in ONE launch; the same cut as two launches gives the same bits
    os.environ["PFMI_QF_TWO_LAUNCHES"] = "1"
    try:
        elbo_t, se_t, best_t = eng.elbo_batch(N, seeds)
        logs_t = eng.elbo_logs(last, N)
    finally:
        os.environ.pop("PFMI_QF_TWO_LAUNCHES", None)
    np.testing.assert_array_equal(logs_a[0], logs_t[0])
    np.testing.assert_array_equal(logs_a[1], logs_t[1])
    np.testing.assert_array_equal(elbo_a, elbo_t)
    np.testing.assert_array_equal(best_a, best_t)
    # the same fits as a 2-path batch on a fresh engine (few fits: the groups of a fit are split over several workgroups)
    e2 = pfmi_mod.Engine(0)
    try:
        e2.set_target(tg)
        e2.optimize_batch(x0[:2], J)
        e2.fit_batch(J)
        elbo_c, se_c, best_c = e2.elbo_batch(N, seeds[:e2.P])
        np.testing.assert_array_equal(elbo_c, elbo_a[:e2.P])
        np.testing.assert_array_equal(best_c, best_a[:2])
    finally:
        e2.close()


# ---- enqueue / wait split and the device-side winner pick -----------------------------------------
def test_enqueue_wait_and_pool_build_best_equal_blocking_calls(pfmi_mod, eng):
    d, J, N, K = 120, 6, 200, 6
    tg = pfmi_mod.t_lowrank(d, r=8, seed=2)
    eng.set_target(tg)
    x0 = pfmi_mod.HostRNG(23).rand(K * d).reshape(K, d) * 4 - 2
    # one path that cannot succeed: starts at the optimum -> L = 0 -> fit_iteration 0, success false (src/singlepath.jl:299)
    x0[2] = tg.mean
    npts = eng.optimize_batch(x0, J, 60)
    assert npts[2] == 1
    eng.fit_batch(J)
    seeds = fit_seeds(eng.P, 9)
    elbo, se, best = eng.elbo_batch(N, seeds)
    fail_seeds = pfmi_mod.hostrng.rand_u64(77, np.arange(K, dtype=np.uint64), 3)
    pts = np.array([int(eng.offsets[k]) + int(best[k]) for k in range(K)])
    ok = np.array([npts[k] > 1 and best[k] > 0 and np.isfinite(elbo[pts[k]]) for k in range(K)])
    assert not ok[2] and ok.sum() == K - 1 and best[2] == 0
    sd = np.where(ok, seeds[pts], fail_seeds)
    eng.pool_build(N, pts, sd)
    pool_ref, lr_ref = eng.pool_get()
    ref = eng.psis(lr_ref)
    idx_ref = eng.resample_indices(K * N, 150, seed=4)
    draws_ref = eng.pool_gather(idx_ref)
    # ---- the same through the enqueue-only entry points: nothing waits until psis_resample's single synchronisation
    e2 = pfmi_mod.Engine(0)
    try:
        e2.set_target(tg)
        e2.optimize_batch_enqueue(x0, J, 60)
        np.testing.assert_array_equal(e2.optimize_batch_wait(), npts)
        e2.fit_batch(J)
        e2.elbo_batch_enqueue(N, seeds)
        e2.pool_build_best(N, fail_seeds)
        comm = pfmi_mod.Comm.init_all([e2])
        res, idx, draws = comm.psis_resample(150, seed=4)
        elbo2, se2, best2 = e2.elbo_batch_wait()
        np.testing.assert_array_equal(elbo2, elbo)
        np.testing.assert_array_equal(se2, se)
        np.testing.assert_array_equal(best2, best)
        p2, s2, ok2 = e2.pool_winners()
        np.testing.assert_array_equal(p2, pts)
        np.testing.assert_array_equal(s2, sd)
        np.testing.assert_array_equal(ok2, ok)
        pool2, lr2 = e2.pool_get()
        np.testing.assert_array_equal(pool2, pool_ref)
        np.testing.assert_array_equal(lr2, lr_ref)
        assert res["pareto_shape"] == ref["pareto_shape"] and res["tail_length"] == ref["tail_length"]
        np.testing.assert_array_equal(idx, idx_ref)
        np.testing.assert_array_equal(draws, draws_ref)
        w, lw = e2.psis_weights(K * N)
        np.testing.assert_array_equal(w, ref["weights"])
        np.testing.assert_array_equal(lw, ref["log_weights"])
        comm.close()
    finally:
        e2.close()


# ---- stage timers: host-synchronised (mode 1) and in-stream (mode 2) ---------------------------------------------------------------
def test_profile_modes_agree_and_do_not_change_results(pfmi_mod):
    """pfmi_profile(ctx, 2) leaves the hipEvent pairs in the stream (the pipeline runs as unprofiled) and pfmi_kernel_time reads them:
    same launch counts as mode 1, times of the same order (mode 1 adds the host's launch latency to every stage), identical results."""
    d, K, J, N = 64, 6, 6, 256
    tg = pfmi_mod.t_lowrank(d, 8, 2)
    x0 = pfmi_mod.HostRNG(4).rand(K * d).reshape(K, d) * 4 - 2
    out = {}
    e = pfmi_mod.Engine(0)
    try:
        e.set_target(tg)
        for mode in (0, 1, 2):
            e.profile(mode)
            e.optimize_batch(x0, J)
            seeds = fit_seeds(e.P, 2)
            for _ in range(3):
                e.fit_batch(J)
                e.elbo_batch_enqueue(N, seeds)
                e.pool_build_best(N, np.arange(K, dtype=np.uint64))
                res = e.elbo_batch_wait()
            out[mode] = (res, {n: e.kernel_time(n) for n in ("optimize", "history", "fit", "elbo_draws", "elbo_draws_x", "elbo_reduce")})
        with pytest.raises(pfmi_mod.PfmiError):
            e.profile(3)
    finally:
        e.close()
    for mode in (1, 2):
        for a, b in zip(out[0][0], out[mode][0]):
            np.testing.assert_array_equal(a, b)
    assert all(v == (0.0, 0) for v in out[0][1].values())
    for name, (ms1, n1) in out[1][1].items():
        ms2, n2 = out[2][1][name]
        assert n1 == n2 and n1 >= 1, (name, n1, n2)
        assert 0.0 < ms2 <= ms1 * 1.5 + 0.05, (name, ms1, ms2)       # in-stream figures carry no launch latency: never much above mode 1


# ---- random shapes: every kernel route against its sibling and the history walk against the oracle -------------------------------------
@pytest.mark.timeout(900)
def test_fuzz_random_shapes_cross_kernel_consistency():
    """tests/probes/fuzz_probe.py with a fixed seed: 40 random (d, J, K, N, target) cases, d from 3 to 7000 -- single-pass scan vs
    lane kernel per draw, register / panel vs memory-resident fit kernel, history walk vs the oracle, on device-made traces."""
    import json
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "probes", "fuzz_probe.py"), "7", "40"], capture_output=True, text=True,
                         timeout=800, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("cases")][-1]
    assert "MISMATCH" not in out.stdout, out.stdout[-2000:]
    assert re.search(r"cases 40 pattern mismatches 0 ", line), line
    worst = json.loads(line[line.index("{"):].replace("'", '"'))
    print(line)
    for key in ("lp", "lq", "elbo", "alpha"):
        assert worst[key] <= 1e-9, (key, worst)
    for key in ("ld", "mu"):
        assert worst[key] <= 1e-7, (key, worst)


def test_callback_target_equals_builtin(pfmi_mod, eng):
    """the host-closure target (reference's general logp, src/elbo.jl:15) gives the built-in target's numbers"""
    tg = pfmi_mod.t_diag(20, seed=3)
    traces = make_traces(tg, 2, 5)
    seeds = None
    out = []
    for target in (tg, pfmi_mod.CallbackTarget(20, lambda x: float(tg.logp(x))),
                   pfmi_mod.CallbackTarget(20, lambda x: float(tg.logp(x)), logp_batch=lambda X: tg.logp(X))):   # vectorised closure
        eng.set_target(target)
        eng.set_traces([t.points for t in traces], [t.gradients for t in traces])
        eng.fit_batch(6)
        seeds = fit_seeds(eng.P, 3)
        out.append(eng.elbo_batch(64, seeds))
        eng.pool_build(70, [int(eng.offsets[k]) + int(out[-1][2][k]) for k in range(2)], [1, 2])
        out[-1] = out[-1] + eng.pool_get()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12, equal_nan=True)


# ---- device-resident logp closures (VERDICT r2 missing #3 / next #3a) ------------------------------------------------------
@pytest.mark.parametrize("shape", [("lowrank", 1000, 6, 1000), ("lowrank", 130, 6, 200), ("diag", 77, 4, 64), ("funnel", 300, 6, 256),
                                   ("lowrank", 3000, 10, 300)])
def test_device_callback_matches_builtin_target_and_oracle(pfmi_mod, eng, shape):
    """The SAME target once as a built-in (logp expanded algebraically, x never formed) and once as a DEVICE closure: the library
    materialises the draws in HBM and the user's HIP kernel (examples/device_logp) evaluates logp there.  ELBO / SE / argmax / per-draw
    logs must agree to roundoff with the built-in route and with the oracle; pool, PSIS and indices follow."""
    tname, d, J, N = shape
    tg = {"lowrank": lambda: pfmi_mod.t_lowrank(d, r=8, seed=2), "diag": lambda: pfmi_mod.t_diag(d, seed=1),
          "funnel": lambda: pfmi_mod.t_funnel(d)}[tname]()
    K = 3
    sc = 2.0
    x0 = pfmi_mod.HostRNG(17).rand(K * d).reshape(K, d) * 2 * sc - sc
    eng.set_target(tg)
    npts = eng.optimize_batch(x0, J, 40)
    traces = [eng.get_trace(k, logp=False) for k in range(K)]
    eng.fit_batch(J)
    seeds = fit_seeds(eng.P, 5)
    elbo0, se0, best0 = eng.elbo_batch(N, seeds)
    logs0 = [eng.elbo_logs(int(eng.offsets[k]) + int(best0[k]), N) for k in range(K)]
    pts = [int(eng.offsets[k]) + int(best0[k]) for k in range(K)]
    eng.pool_build(N, pts, seeds[pts])
    pool0, lr0 = eng.pool_get()
    # ---- the device closure
    dtg = demo_device_target(tg)
    e2 = pfmi_mod.Engine(0)
    try:
        e2.set_target(dtg)
        e2.set_traces([t[0] for t in traces], [t[2] for t in traces])
        e2.fit_batch(J)
        tables = []
        # one block / many small blocks of fits, the blocks alternating between two streams (round 6: the closure of block i runs beside the writer
        # of block i + 1) or all on one stream: the same bits every time
        for chunk_mb, overlap in ((None, None), ("0.5", None), ("0.5", "0"), (None, "0")):
            if chunk_mb:
                os.environ["PFMI_DEVCB_CHUNK_MB"] = chunk_mb
            if overlap:
                os.environ["PFMI_DEVCB_OVERLAP"] = overlap
            try:
                elbo1, se1, best1 = e2.elbo_batch(N, seeds)
            finally:
                os.environ.pop("PFMI_DEVCB_CHUNK_MB", None)
                os.environ.pop("PFMI_DEVCB_OVERLAP", None)
            tables.append((elbo1.copy(), se1.copy(), np.concatenate([e2.elbo_logs(p, N)[0] for p in range(1, min(e2.P, 6))])))
            assert e2.callback_stats_dev()["bytes_in_hbm"] == 8.0 * d * N * (e2.P - K)
            fin = np.isfinite(elbo0)
            np.testing.assert_array_equal(np.isfinite(elbo1), fin)
            assert np.max(np.abs(elbo1[fin] - elbo0[fin]) / (1 + np.abs(elbo0[fin]))) <= 1e-9
            assert np.max(np.abs(se1[fin] - se0[fin]) / (1 + se0[fin])) <= 1e-8
            np.testing.assert_array_equal(best1, best0)
        for t in tables[1:]:
            for a, b in zip(tables[0], t):
                np.testing.assert_array_equal(a, b)
        for k in range(K):
            lp1, lq1 = e2.elbo_logs(pts[k], N)
            assert np.max(np.abs(lq1 - logs0[k][1]) / (1 + np.abs(lq1))) <= 1e-13      # same normals; |u|^2 summed in another order
            assert np.max(np.abs(lp1 - logs0[k][0]) / (1 + np.abs(logs0[k][0]))) <= 1e-9
        e2.pool_build(N, pts, seeds[pts])
        pool1, lr1 = e2.pool_get()
        # same normals, same factor; the built-in route may use another writer (two-pass kernel for d <= 1024): roundoff apart
        assert np.max(np.abs(pool1 - pool0) / (1 + np.abs(pool0).max(axis=0))) <= 1e-10
        assert np.max(np.abs(lr1 - lr0) / (1 + np.abs(lr0))) <= 1e-9
        for k in range(K):                                        # within ONE target a draw is the same bits alone or in the pool
            Xk, _, _ = e2.draws(pts[k], seeds[pts[k]], 3, n0=7)
            np.testing.assert_array_equal(Xk, pool1[:, 7:10, k])
        # against the closure evaluated on the host copy of the same draws, and pfmi_draws through the closure
        X, lpd, lqd = e2.draws(pts[0], seeds[pts[0]], 50)
        assert np.max(np.abs(lpd - tg.logp(X)) / (1 + np.abs(lpd))) <= 1e-11
    finally:
        e2.close()
    # oracle, path 0
    ref = po.path_fit_elbo(traces[0][0], traces[0][2], J, oracle_target(tg), N, seeds[:int(eng.offsets[1])])
    y = ref["elbo"][1:]
    x = elbo1[1:int(eng.offsets[1])]
    ok = np.isfinite(y)
    assert np.all(np.abs(x[ok] - y[ok]) <= 8 * ref["se"][1:][ok] + 1e-8 * (1 + np.abs(y[ok])))


def test_device_callback_failed_fits_and_torch_closure(pfmi_mod):
    """(i) failed fits stay NaN through the device-closure route (their draws do not exist); (ii) a closure written with torch ops
    on the engine's stream (pfmi.TorchDeviceTarget) == the host closure on the same draws."""
    import torch
    d, J, N = 40, 5, 128
    rng = np.random.default_rng(0)
    bad_th, bad_gr = np.cumsum(rng.normal(size=(9, d)), 0), rng.normal(size=(9, d))
    tg = pfmi_mod.t_diag(d, seed=3)
    good = make_traces(tg, 2, 3)
    e = pfmi_mod.Engine(0)
    try:
        m = torch.as_tensor(tg.mean, device="cuda:0")
        a = torch.as_tensor(tg.a, device="cuda:0")
        ttg = pfmi_mod.TorchDeviceTarget(d, lambda X: -0.5 * (((X - m) ** 2) * a).sum(1), host=tg)
        for target in (demo_device_target(tg), ttg):
            e.set_target(target)
            e.set_traces([bad_th] + [t.points for t in good], [bad_gr] + [t.gradients for t in good])
            e.fit_batch(J, -1e300)                               # negative-curvature pairs accepted: non-PD fits (src/woodbury.jl:202,205)
            status = e.fit_status()[0]
            assert np.any(status != 0) and np.any(status == 0)
            seeds = fit_seeds(e.P, 2)
            elbo, se, best = e.elbo_batch(N, seeds)
            for p in range(e.P):
                lp, lq = e.elbo_logs(p, N)
                first = p in e.offsets[:-1]
                if status[p] != 0:
                    assert np.all(np.isnan(lp)) and np.all(np.isnan(lq)) and np.isnan(elbo[p])
                elif not first:
                    X, _, lq2 = e.draws(p, seeds[p], N)
                    np.testing.assert_array_equal(lq, lq2)
                    assert np.max(np.abs(lp - tg.logp(X)) / (1 + np.abs(lp))) <= 1e-12
    finally:
        e.close()


def test_python_closures_that_raise_are_reraised(pfmi_mod):
    """An exception inside a Python logp closure (host callback or torch device closure) used to be printed and swallowed by ctypes,
    leaving stale memory to be reduced into ELBOs: it now fills its block with NaN and is re-raised by the Engine call."""
    d, J = 20, 4
    calls = {"n": 0}

    def bad(x):
        calls["n"] += 1
        if calls["n"] > 3:
            raise ZeroDivisionError("closure failed")
        return float(-0.5 * (x @ x))

    tg = pfmi_mod.CallbackTarget(d, bad, grad=lambda x: -x)
    good = pfmi_mod.t_iso(d)
    eng = pfmi_mod.Engine(0)
    try:
        tr = pfmi_mod.optimize_with_trace(good, pfmi_mod.HostRNG(1).rand(d) * 4 - 2, history_length=J)
        eng.set_target(tg)
        eng.set_traces([tr.points], [tr.gradients])
        eng.fit_batch(J)
        with pytest.raises(ZeroDivisionError):
            eng.elbo_batch(16, fit_seeds(eng.P, 1))
        assert tg.pending_error is None                                  # consumed: the next call starts clean
        import torch

        def tbad(X):
            raise RuntimeError("torch closure failed")

        tt = pfmi_mod.TorchDeviceTarget(d, tbad, host=good)
        eng.set_target(tt)
        eng.set_traces([tr.points], [tr.gradients])
        eng.fit_batch(J)
        with pytest.raises(RuntimeError, match="torch closure failed"):
            eng.elbo_batch(16, fit_seeds(eng.P, 1))
        assert torch.cuda.is_available()
    finally:
        eng.close()


@pytest.mark.timeout(900)
def test_scan_handover_under_contention_is_bit_identical_and_never_gives_up():
    rc, out = _run([sys.executable, PROBE, "200", "--contend"], 800)
    assert rc == 0, out
    assert "give-up counter 0" in out and " 0 differ" in out, out


@pytest.mark.timeout(900)
def test_scan_handover_under_rocprofv3_kernel_trace():
    exe = shutil.which("rocprofv3")
    if not exe:
        pytest.skip("rocprofv3 not on PATH")
    rc, out = _run([exe, "--kernel-trace", "-d", "/tmp/pfmi_stress_prof", "-o", "s", "--", sys.executable, PROBE, "60", "--contend"], 800)
    shutil.rmtree("/tmp/pfmi_stress_prof", ignore_errors=True)
    assert rc == 0, out
    assert "give-up counter 0" in out and " 0 differ" in out, out


def test_handover_timeout_is_retryable_and_switches_to_the_wait_free_cut(pfmi_mod):
    """PFMI_QF_FAKE_LOST=1: the first wait of a context reports one lost piece.  pfmi_elbo_batch_wait returns PFMI_ERR_RETRY, the context
    takes the two-launch cut from then on, and multipathfinder / pathfinder re-enqueue with the same seeds: the same result as an
    undisturbed call."""
    L = pfmi_mod.lib()
    tg = pfmi_mod.t_lowrank(300, r=8, seed=2)
    kw = dict(nruns=6, ndraws_elbo=1000, history_length=6, maxiters=60)
    e0 = pfmi_mod.Engine(0)
    ref = pfmi_mod.multipathfinder(tg, 200, rng=pfmi_mod.HostRNG(5), engine=e0, **kw)
    ref1 = pfmi_mod.pathfinder(tg, ndraws=50, ndraws_elbo=1000, rng=pfmi_mod.HostRNG(6), engine=e0, maxiters=60)
    e0.close()
    assert L.pfmi_debug_set(b"PFMI_QF_FAKE_LOST", b"1") == 0
    try:
        e1 = pfmi_mod.Engine(0)
        e1.set_target(tg)
        x0 = pfmi_mod.HostRNG(3).rand(4 * 300).reshape(4, 300) * 4 - 2
        npts = e1.optimize_batch(x0, 6, 60)
        e1.fit_batch(6)
        sd = np.arange(e1.P, dtype=np.uint64) + np.uint64(7)
        with pytest.raises(pfmi_mod._lib.PfmiRetry):
            e1.elbo_batch(1000, sd)
        assert e1.kernel_time("qf_handover_lost")[1] == 1
        a = e1.elbo_batch(1000, sd)                                 # second attempt: the wait-free cut, no error
        e1.close()
        e2 = pfmi_mod.Engine(0)                                     # a fresh context trips once inside the public call ...
        got = pfmi_mod.multipathfinder(tg, 200, rng=pfmi_mod.HostRNG(5), engine=e2, **kw)
        assert e2.kernel_time("qf_handover_lost")[1] == 1           # ... which retried
        e2.close()
        e3 = pfmi_mod.Engine(0)
        got1 = pfmi_mod.pathfinder(tg, ndraws=50, ndraws_elbo=1000, rng=pfmi_mod.HostRNG(6), engine=e3, maxiters=60)
        assert e3.kernel_time("qf_handover_lost")[1] == 1
        e3.close()
    finally:
        assert L.pfmi_debug_set(b"PFMI_QF_FAKE_LOST", None) == 0
    np.testing.assert_array_equal(got.draws, ref.draws)
    np.testing.assert_array_equal(got.draw_component_ids, ref.draw_component_ids)
    assert got.psis_result.pareto_shape == ref.psis_result.pareto_shape
    np.testing.assert_array_equal(got1.draws, ref1.draws)
    assert got1.fit_iteration == ref1.fit_iteration
    e4 = pfmi_mod.Engine(0)                                         # and the undisturbed scan of the same fits equals the wait-free cut's
    e4.set_target(tg)
    e4.optimize_batch(x0, 6, 60)
    e4.fit_batch(6)
    b = e4.elbo_batch(1000, sd)
    e4.close()
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[2], b[2])
    assert int(npts.sum()) > 4
