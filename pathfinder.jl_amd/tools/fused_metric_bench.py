"""The metric windows on a built-in target inside the fused kernels (pfmi_hmc_fused_metric_enqueue, pfmi_nuts_fused_metric_enqueue) beside
what the same chains had before: three routes, one adaptive run each (W warm-up transitions with the metric windows of csrc/adapt.h, then T
sampling transitions), INTERLEAVED in one process per step:
  (a) the new route on the built-in target;
  (b) pfmi_*_adapt_metric_enqueue on the example HIP closure of examples/device_logp that restates the same density (tests/helpers.py:
      demo_device_target(tg, grad=True)) -- the route a user had for the adapted metric: one closure call and one step launch per round;
  (c) pfmi_*_fused_enqueue with the same W and T and no windows: what the fused route cost before, so that (a) - (c) is what the scale
      and the whiten pass cost.
Shapes: t_lowrank(1000, r=8) and t_funnel(1000), J = 6, K = 64, 256, 1024 chains, W = 150, T = 200, nleapfrog 8 / max_depth 8, every chain
on the best fit of one path from that fit's trace point, step size d^(-1/4) (static HMC: half of it), the same seeds on all routes.

Every step -- (sampler, target), then the launch cap -- is a CHILD process under a time limit of its own; a step that fails or runs out
of time ends the run: nothing is tried again and nothing more is started.  Per step one unmeasured run of each route, then --reps
interleaved triples; one JSON line per K:
  * wall_ms        HOST clock from the enqueue to the return of the wait, [median, min, max] per route
  * a_over_b       (b) wall / (a) wall (medians); a_wins: the [min, max] of (a) lies wholly below that of (b)
  * a_minus_c_us   ((a) - (c)) wall per transition and launch, microseconds: the cost of the scale and the whiten pass
  * ess_per_s      minimum bulk ESS over the coordinates (pfmi_chain_diagnostics of the resident draws) / wall seconds, (a) and (c)
  * accept, eps    mean acceptance and the range of the adapted step sizes of each route; status: the OR of the chains' PFMI_ADAPT_* bits
and, for --cap-K chains, one line for the launch cap of route (a): caps 1024 and uncut, interleaved, and the relative cost of 1024.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
STEP_LIMIT = 420                                                # seconds, per child


def stat(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def step(a):
    """one child: a sampler on a target, every K (or the cap line)"""
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)                                   # (tests/helpers.py imports the oracle package)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pfmi
    from helpers import demo_device_target
    from hmc_fused_bench import setup as setup_gauss

    def setup(eng, target, d, J, K):
        """hmc_fused_bench.setup; the funnel's path starts where the tests' funnel paths start (tests/hmc_reference.py: grid_path_x0)"""
        if a.target != "funnel":
            return setup_gauss(eng, target, d, J, K)
        import hmc_reference as H
        eng.set_target(target)
        npts = eng.optimize_batch(H.grid_path_x0(pfmi, "funnel", d), J, 40, 1e-8)
        eng.fit_batch(J)
        _, _, best = eng.elbo_batch(64, pfmi.hostrng.rand_u64(5, np.arange(int(npts[0]), dtype=np.uint64), 9))
        p = int(best[0])
        th, _, _ = eng.get_trace(0)
        return np.full(K, p, dtype=np.int64), np.asfortranarray(np.repeat(th[p][:, None], K, axis=1))

    d, W, T, nuts = a.d, a.W, a.T, a.sampler == "nuts"
    tg = pfmi.t_funnel(d) if a.target == "funnel" else pfmi.t_lowrank(d, a.r, 2)
    param = a.max_depth if nuts else a.nleapfrog
    eps = d ** -0.25 * (1.0 if nuts else 0.5)
    L = pfmi._lib.lib()
    fe, ce = pfmi.Engine(0), pfmi.Engine(0)                    # the built-in target; the closure that restates it

    def cap(n):
        L.pfmi_debug_set(b"PFMI_NUTS_FUSED_ROUNDS" if nuts else b"PFMI_HMC_FUSED_ROUNDS", None if n is None else str(n if n else 2 ** 31 - 1).encode())

    def timed(eng, enqueue):
        t0 = time.perf_counter()
        enqueue()
        eng.nuts_wait() if nuts else eng.hmc_wait()
        return (time.perf_counter() - t0) * 1e3

    def facts(eng):
        warm = eng.adapt_get()
        return {"accept": round(float(eng.hmc_get(draws=False)["accept_prob"].mean()), 3),
                "eps": [round(float(warm["step_size"].min()), 4), round(float(warm["step_size"].max()), 4)],
                "status": int(np.bitwise_or.reduce(warm["status"])), "ess": float(np.min(eng.chain_diagnostics()["ess_bulk"]))}

    try:
        if a.caps:
            K = a.cap_K
            fp, fx = setup(fe, tg, d, a.J, K)
            seeds = pfmi.HostRNG(17).rand_u64(K)
            new = lambda: (fe.nuts_fused_metric_enqueue if nuts else fe.hmc_fused_metric_enqueue)(fp, fx, seeds, eps, param, T, nwarmup=W)   # noqa: E731
            walls = {c: [] for c in (1024, 0)}
            for c in walls:
                cap(c); timed(fe, new)
            for _ in range(a.reps):
                for c in walls:
                    cap(c)
                    walls[c].append(timed(fe, new))
            cap(None)
            rel = float(np.median(walls[1024]) / np.median(walls[0]) - 1.0)
            print(json.dumps({"sampler": a.sampler, "target": a.target, "K": K, "caps": {"1024": stat(walls[1024]), "uncut": stat(walls[0])},
                              "cap_1024_cost": round(rel, 5), "under_one_percent": bool(rel < 0.01), "clock": "host"}), flush=True)
            return
        for K in a.K:
            fp, fx = setup(fe, tg, d, a.J, K)
            cp, cx = setup(ce, demo_device_target(tg, grad=True), d, a.J, K)
            seeds = pfmi.HostRNG(17).rand_u64(K)
            if nuts:
                ra = lambda: fe.nuts_fused_metric_enqueue(fp, fx, seeds, eps, param, T, nwarmup=W)           # noqa: E731
                rb = lambda: ce.nuts_adapt_metric_enqueue(cp, cx, seeds, eps, param, W, T)                   # noqa: E731
                rc = lambda: fe.nuts_fused_enqueue(fp, fx, seeds, eps, param, T, nwarmup=W)                  # noqa: E731
            else:
                ra = lambda: fe.hmc_fused_metric_enqueue(fp, fx, seeds, eps, param, T, nwarmup=W)            # noqa: E731
                rb = lambda: ce.hmc_adapt_metric_enqueue(cp, cx, seeds, eps, param, W, T)                    # noqa: E731
                rc = lambda: fe.hmc_fused_enqueue(fp, fx, seeds, eps, param, T, nwarmup=W)                   # noqa: E731
            routes = (("a", fe, ra), ("b", ce, rb), ("c", fe, rc))
            for _, eng, run in routes:
                timed(eng, run)
            walls, fact = {q: [] for q, _, _ in routes}, {}
            for _ in range(a.reps):
                for q, eng, run in routes:
                    walls[q].append(timed(eng, run))
                    fact[q] = facts(eng)
            med = {q: float(np.median(v)) for q, v in walls.items()}
            ess = {q: fact[q].pop("ess") for q in fact}
            launches = (W + T) * (a.nleapfrog if not nuts else 1)
            print(json.dumps({"sampler": a.sampler, "target": a.target, "K": K, "d": d, "J": a.J, "W": W, "T": T, "param": param, "reps": a.reps,
                              "wall_ms": {q: stat(v) for q, v in walls.items()}, "clock": "host",
                              "a_over_b": round(med["b"] / med["a"], 2), "a_wins": bool(max(walls["a"]) < min(walls["b"])),
                              "a_over_c": round(med["a"] / med["c"], 3),
                              "a_minus_c_us": round((med["a"] - med["c"]) * 1e3 / launches, 3), "per": "round" if not nuts else "transition",
                              "ess_per_s": {q: round(ess[q] / (med[q] * 1e-3), 1) for q in ("a", "c")}, "min_ess_bulk": {q: round(ess[q], 1) for q in ess},
                              "facts": fact}), flush=True)
    finally:
        cap(None)
        fe.close(); ce.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--W", type=int, default=150)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--nleapfrog", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap-K", type=int, default=64)
    ap.add_argument("--samplers", nargs="+", default=["hmc", "nuts"])
    ap.add_argument("--targets", nargs="+", default=["lowrank", "funnel"])
    ap.add_argument("--sampler")
    ap.add_argument("--target")
    ap.add_argument("--caps", action="store_true")
    a = ap.parse_args()
    if a.sampler:                                               # a child
        return step(a)
    base = [sys.executable, os.path.abspath(__file__)] + [x for x in sys.argv[1:]]
    steps = [(s, t, False) for s in a.samplers for t in a.targets] + [(s, "lowrank", True) for s in a.samplers]
    for s, t, caps in steps:
        try:
            rc = subprocess.run(base + ["--sampler", s, "--target", t] + (["--caps"] if caps else []), timeout=STEP_LIMIT).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                             # no retry, and nothing more on the GPU after a failed step
            print(json.dumps({"failed": [s, t, caps], "returncode": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
