"""What the metric windows cost per launch (profiles/metric_adapt.md): the metric kernels (pfmi_hmc_adapt_metric_enqueue /
pfmi_nuts_adapt_metric_enqueue: a per-coordinate scale in every kick and drift, the whiten pass and the Welford update after a window
transition) beside the warm kernels (pfmi_hmc_adapt_enqueue / pfmi_nuts_adapt_enqueue), in one process on the same fit, starts and seeds.

  python tools/metric_adapt_bench.py [--K 64 --d 1000 --J 6 --nwarmup 200 --reps 5]

One JSON line per sampler: round_us = hipEvent time of the stage ("hmc_metric" / "hmc_adapt", ...) per launch over a run of nwarmup
warm-up transitions and one sampling transition (median, min, max over reps), the launches of a run, and the final step sizes of both."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pfmi  # noqa: E402
from closure_lbfgs_bench import hip_target  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--nleapfrog", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--nwarmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    K, d, W = a.K, a.d, a.nwarmup
    tg = pfmi.t_lowrank(d, 8, 2)
    eng = pfmi.Engine(0)
    eng.set_target(hip_target(tg))
    x0 = pfmi.HostRNG(3).rand(d).reshape(1, d) * 4 - 2
    npts = eng.optimize_batch(x0, a.J, 200, 1e-8)
    eng.fit_batch(a.J)
    _, _, best = eng.elbo_batch(64, pfmi.hostrng.rand_u64(5, np.arange(int(npts[0]), dtype=np.uint64), 9))
    p = int(best[0])
    th, _, _ = eng.get_trace(0)
    pts = np.full(K, p, dtype=np.int64)
    X0 = np.asfortranarray(np.repeat(th[p][:, None], K, axis=1))
    seeds = pfmi.HostRNG(17).rand_u64(K)
    eps0 = np.full(K, d ** -0.25)
    for sampler, param in (("hmc", a.nleapfrog), ("nuts", a.max_depth)):
        wait = eng.hmc_wait if sampler == "hmc" else eng.nuts_wait
        runs = {"adapt": eng.hmc_adapt_enqueue if sampler == "hmc" else eng.nuts_adapt_enqueue,
                "metric": eng.hmc_adapt_metric_enqueue if sampler == "hmc" else eng.nuts_adapt_metric_enqueue}
        out = {"sampler": sampler, "d": d, "K": K, "nwarmup": W, "param": param, "reps": a.reps, "round_us": {}, "launches": {}, "step_size": {}}
        eng.profile(2)
        for which, enq in runs.items():
            stage, us = "%s_%s" % (sampler, which), []
            for rep in range(a.reps + 1):
                m0, n0 = eng.kernel_time(stage)
                enq(pts, X0, seeds, eps0, param, W, 1)
                wait()
                m1, n1 = eng.kernel_time(stage)
                if rep:
                    us.append((m1 - m0) / (n1 - n0) * 1e3)
            eps = eng.adapt_get()["step_size"]
            out["round_us"][which] = [round(float(np.median(us)), 3), round(float(np.min(us)), 3), round(float(np.max(us)), 3)]
            out["launches"][which] = int(n1 - n0)
            out["step_size"][which] = [round(float(eps.min()), 4), round(float(eps.max()), 4)]
        eng.profile(0)
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
