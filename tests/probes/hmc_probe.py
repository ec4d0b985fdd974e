"""Device HMC with the fitted metric (pfmi_hmc_enqueue) at the headline shape -- d = 1000, J = 6, K = 64 chains, Lf = 8, T = 50 on the
example Gaussian closure of examples/device_logp -- against the only route the library offered before: a leapfrog driven from the
host over pfmi_woodbury_apply(PFMI_OP_MUL), the closure evaluated through the existing entry points.  Writes its table as
markdown to the path given as the first argument (default: profiles/hmc.md).

  per-round device times   pfmi_kernel_time("hmc") and ("hmc_closure") under pfmi_profile mode 2 (event pairs left in the stream), a
                           run of its own; the step kernel's nominal bytes per round over its time
  wall time                host clock around enqueue + wait, profiling off, REPEATS repeats after WARMUP warm-up calls, best and median
  baseline                 plain-momentum leapfrog p += e grad logp(x), x += e Sigma p on the host: Sigma p is ONE pfmi_woodbury_apply
                           (PFMI_OP_MUL, N = K columns: every chain on the same fit, the baseline's best case), the gradient comes from a
                           second engine through pfmi_optimize_batch(maxiters = 0) + pfmi_get_trace (the only entry points that run the
                           gradient closure); momentum refresh, energies and the accept step in NumPy.  A few transitions are timed.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "pathfinder.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np                                         # noqa: E402
import pfmi                                                # noqa: E402
from helpers import demo_device_target, fit_seeds          # noqa: E402

D, J, K, LF, T = 1000, 6, 64, 8, 50
WARMUP, REPEATS, BASE_T = 2, 7, 3
KPAD = 12
HBM_GBPS = 8000.0


def main(out_path):
    tg = pfmi.t_lowrank(D, r=8, seed=2, wscale=2.0 / np.sqrt(D))
    eng = pfmi.Engine(0)
    eng.set_target(demo_device_target(tg, grad=True))
    x0p = pfmi.HostRNG(2024).rand(4 * D).reshape(4, D) * 4 - 2
    npts = eng.optimize_batch(x0p, J, 200)
    eng.fit_batch(J)
    status, jeff, _, _ = eng.fit_status()
    _, _, best = eng.elbo_batch(64, fit_seeds(eng.P, 3))
    p = int(eng.offsets[0]) + int(best[0])
    assert status[p] == 0
    th, _, _ = eng.get_trace(0)
    rng = np.random.default_rng(5)
    x0 = np.asfortranarray(th[int(best[0])][:, None] + eng.woodbury_apply(p, "unwhiten", rng.standard_normal((D, K))))
    seeds = np.asarray(pfmi.hostrng.rand_u64(99, np.arange(K, dtype=np.uint64), 9), dtype=np.uint64)
    pts = np.full(K, p, dtype=np.int64)
    eps = 0.6 * D ** -0.25

    def run():
        eng.hmc_enqueue(pts, x0, seeds, eps, LF, T)
        eng.hmc_wait()

    for _ in range(WARMUP):
        run()
    wall = []
    for _ in range(REPEATS):
        eng.sync()
        t0 = time.perf_counter()
        run()
        wall.append(time.perf_counter() - t0)
    got = eng.hmc_get(draws=False)
    rounds, cols = eng.hmc_stats()
    # ---- device times per round, a run of its own under profile mode 2
    eng.profile(2)
    run()
    ms_step, n_step = eng.kernel_time("hmc")
    ms_clo, n_clo = eng.kernel_time("hmc_closure")
    eng.profile(0)
    res = eng.kernel_time("hmc:%d:res" % KPAD)[1] > 0
    # nominal HBM bytes of one step launch, all chains: the factor rows once (LDS-resident), sqrt(alpha), the closure's gradient, the
    # trial point read and written, v read and written, wt written and read back
    bytes_round = K * (D * KPAD * 8 + 8 * D * (1 + 1 + 2 + 2 + 2))
    # ---- the baseline: host leapfrog over pfmi_woodbury_apply(MUL) + the gradient through a second engine
    eng_g = pfmi.Engine(0)
    eng_g.set_target(demo_device_target(tg, grad=True))

    split = {"grad": 0.0, "apply": 0.0}                      # host seconds inside the gradient route / inside pfmi_woodbury_apply

    def apply(op, X):
        t = time.perf_counter()
        out = eng.woodbury_apply(p, op, X)
        split["apply"] += time.perf_counter() - t
        return out

    def grad(X):
        t = time.perf_counter()
        eng_g.optimize_batch(np.ascontiguousarray(X.T), J, 0)
        lp, g = np.empty(K), np.empty((D, K))
        for k in range(K):
            _, l, gr = eng_g.get_trace(k)
            lp[k], g[:, k] = l[0], gr[0]
        split["grad"] += time.perf_counter() - t
        return lp, g

    def base_transitions(n):
        x = x0.copy()
        lp, g = grad(x)
        acc = 0
        for t in range(n):
            pm = apply("invunwhiten", rng.standard_normal((D, K)))  # p = R \ z ~ N(0, Sigma^-1): one more apply per transition
            h0 = -lp + 0.5 * apply("quad", pm)
            xt, gt, lpt = x.copy(), g, lp
            pm = pm + 0.5 * eps * gt
            for i in range(LF):
                xt = xt + eps * apply("mul", pm)
                lpt, gt = grad(xt)
                pm = pm + (eps if i < LF - 1 else 0.5 * eps) * gt
            h1 = -lpt + 0.5 * apply("quad", pm)
            ok = rng.random(K) < np.exp(np.minimum(0.0, h0 - h1))
            x[:, ok], lp[ok], g[:, ok] = xt[:, ok], lpt[ok], gt[:, ok]
            acc += ok.sum()
        return acc / (n * K)

    base_transitions(1)
    eng.sync()
    split["grad"] = split["apply"] = 0.0
    t0 = time.perf_counter()
    base_acc = base_transitions(BASE_T)
    base = (time.perf_counter() - t0) / BASE_T
    base_grad, base_apply = split["grad"] / BASE_T, split["apply"] / BASE_T
    eng_g.close()
    w_best, w_med = min(wall), float(np.median(wall))
    per_tr = w_med / T
    us_step, us_clo = 1e3 * ms_step / max(n_step, 1), 1e3 * ms_clo / max(n_clo, 1)
    gbps = bytes_round / (us_step * 1e-6) / 1e9
    # ONE conclusion.  Traffic bounds the round only if the step kernel's nominal bytes come near the HBM rate; otherwise a round is two
    # dependent, latency-long launches.  The event pairs cannot split a launch's latency from its kernel's run time (profiled, the two
    # device figures add up to more than the unprofiled wall time per round), so no finer attribution is made.
    if gbps > 0.5 * HBM_GBPS:
        bound = "factor and vector traffic of the step kernel"
    else:
        bound = "launch latency: two dependent launches per round (closure, then step kernel), each a few launch latencies long"
    rec = dict(d=D, J=J, K=K, Lf=LF, T=T, eps=eps, rounds=rounds, closure_columns=cols, lds_resident=bool(res), wall_s=wall,
               wall_best_s=w_best, wall_median_s=w_med, ms_per_transition=1e3 * per_tr, step_us_per_round=us_step, closure_us_per_round=us_clo,
               step_launches=n_step, step_bytes_per_round=bytes_round, step_GBps=bytes_round / (us_step * 1e-6) / 1e9,
               accept_mean=float(got["accept_prob"].mean()), divergent=int(got["divergent"].sum()), baseline_ms_per_transition=1e3 * base,
               baseline_transitions=BASE_T, baseline_grad_ms=1e3 * base_grad, baseline_apply_ms=1e3 * base_apply, baseline_accept=float(base_acc), ratio_to_baseline=base / per_tr, bound=bound)
    print("HMC_PROBE", json.dumps(rec))
    lines = [
        "# Device HMC with the fitted Woodbury metric: what a round costs", "",
        "Written by `tests/probes/hmc_probe.py` on an MI355X.  Workload: d = %d, J = %d (column padding %d), K = %d chains on one fit, Lf = %d,"
        % (D, J, KPAD, K, LF),
        "T = %d transitions (%d rounds, %d closure columns), the example Gaussian closure of `examples/device_logp`, step size %.3g"
        % (T, rounds, cols, eps),
        "(mean acceptance %.2f, %d divergent).  Factor rows %s." % (rec["accept_mean"], rec["divergent"], "staged in LDS" if res else "streamed"), "",
        "| quantity | value | source |", "|---|---|---|",
        "| wall time of enqueue + wait | best %.2f ms, median %.2f ms of %d (after %d warm-up calls) | host clock, profiling off |"
        % (1e3 * w_best, 1e3 * w_med, REPEATS, WARMUP),
        "| wall time per transition | %.1f us | median / T |" % (1e6 * per_tr),
        "| wall time per round | %.1f us | median / rounds |" % (1e6 * w_med / rounds),
        "| step kernel per round | %.1f us (%d launches) | `pfmi_kernel_time(\"hmc\")`, profile mode 2, a run of its own |" % (us_step, n_step),
        "| closure kernel per round | %.1f us | `pfmi_kernel_time(\"hmc_closure\")`, same run |" % us_clo,
        "| step kernel nominal traffic per round | %.2f MB -> %.0f GB/s | K (d KPAD 8 B factor rows once + 8 d (s, g, x~ r/w, v r/w, wt w/r)) over its time |"
        % (bytes_round / 1e6, rec["step_GBps"]),
        "| baseline: host leapfrog over `pfmi_woodbury_apply(MUL)` | %.1f ms per transition (%d timed, acceptance %.2f) | host clock |"
        % (1e3 * base, BASE_T, base_acc),
        "| of which: the gradient route (second engine, `pfmi_get_trace` per chain) | %.1f ms per transition | host clock inside the calls |" % (1e3 * base_grad),
        "| of which: the `pfmi_woodbury_apply` calls (Lf + 3 per transition) | %.1f ms per transition | host clock inside the calls |" % (1e3 * base_apply),
        "| ratio baseline / device | %.0fx (the applies alone: %.0fx) | |" % (rec["ratio_to_baseline"], base_apply / per_tr), "",
        "What bounds a round at this shape: **%s**." % bound,
        "The step kernel moves its nominal bytes at %.0f GB/s, %.0f %% of the 8 TB/s HBM rate, so factor traffic does not bound it; the closure's"
        % (gbps, 100 * gbps / HBM_GBPS),
        "kernel is as short.  Profiled, the two device figures add up to %.1f us, more than the %.1f us of an unprofiled round: the event pairs"
        % (us_step + us_clo, 1e6 * w_med / rounds),
        "cannot separate a launch's latency from its kernel's run time, so the split between the two was not measured.", "",
        "The baseline is the parent's only route to the same transitions: per leapfrog step one `pfmi_woodbury_apply` (N = K columns on one fit --",
        "its best case; chains on different fits need one call each) with its PCIe round trip, and the gradient closure through a second",
        "engine (`pfmi_optimize_batch` with maxiters = 0, then `pfmi_get_trace` per chain), the only entry points that evaluate it.  Most of",
        "the baseline's time is that gradient route (K downloads per leapfrog step), not the applies: the ratio is what the call replaces end",
        "to end, not the gain of the step kernel over `pfmi_woodbury_apply`.",
        "Not measured: the step kernel under `rocprofv3` (the figures above are the library's own event pairs), other shapes, chains on",
        "distinct fits.", ""]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hmc.md"))
