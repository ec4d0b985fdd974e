"""NUTS on the fitted metric (pfmi_nuts_enqueue) beside static HMC (pfmi_hmc_enqueue), in one process on the same fits and starts.

Shape: d = 1000, K = 64 chains, J = 6, the example HIP closure of examples/device_logp on t_lowrank(1000, 8, 2); every chain uses the best
fit of one closure-optimised path and starts at that fit's trace point.  The step size is adapted per chain as pfmi.nuts does it (dual
averaging between windows of 10 warm-up transitions).  One JSON line:
  * static_round_us   host clock of an hmc_enqueue + hmc_wait of T transitions of Lf leapfrog steps, per round (1 + T Lf rounds)
  * nuts_round_us     host clock of a nuts_enqueue + nuts_wait of T transitions at the adapted step sizes, per round issued
  * idle_share        share of the closure's columns that belonged to chains that had finished (or to rounds issued ahead of the last
                      progress word): 1 - sum_k (1 + sum_t n_leapfrog[k, t]) / closure columns
  * transitions_per_s K T / wall time of the NUTS call
  * tree_depth, n_leapfrog   means over the sampling call; step_size the adapted range
Medians of --reps calls after one warm-up call."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pfmi  # noqa: E402
from closure_lbfgs_bench import hip_target  # noqa: E402
from pfmi.hmc import dual_averaging_init, dual_averaging_update  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--nleapfrog", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--nwarmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    K, d = a.K, a.d
    tg = pfmi.t_lowrank(d, 8, 2)
    eng = pfmi.Engine(0)
    eng.set_target(hip_target(tg))
    x0 = pfmi.HostRNG(3).rand(d).reshape(1, d) * 4 - 2
    npts = eng.optimize_batch(x0, a.J, 200, 1e-8)
    eng.fit_batch(a.J)
    seeds_fit = pfmi.hostrng.rand_u64(5, np.arange(int(npts[0]), dtype=np.uint64), 9)
    _, _, best = eng.elbo_batch(64, seeds_fit)
    p = int(best[0])
    th, _, _ = eng.get_trace(0)
    pts = np.full(K, p, dtype=np.int64)
    X0 = np.asfortranarray(np.repeat(th[p][:, None], K, axis=1))
    seeds = pfmi.HostRNG(17).rand_u64(K)

    # the step sizes pfmi.nuts would sample with
    eps = np.full(K, d ** -0.25)
    state, done = dual_averaging_init(eps), 0
    ebar = eps
    while done < a.nwarmup:
        eng.nuts_enqueue(pts, X0, seeds, eps, a.max_depth, 10, cont=done > 0)
        eng.nuts_wait()
        done += 10
        state, eps, ebar = dual_averaging_update(state, eng.hmc_get(draws=False)["accept_prob"].mean(axis=1), 0.8)
    eps = np.asarray(ebar)

    def static():
        t0 = time.perf_counter()
        eng.hmc_enqueue(pts, X0, seeds, eps, a.nleapfrog, a.T)
        eng.hmc_wait()
        return time.perf_counter() - t0, eng.hmc_stats()

    def nuts():
        t0 = time.perf_counter()
        eng.nuts_enqueue(pts, X0, seeds, eps, a.max_depth, a.T)
        eng.nuts_wait()
        return time.perf_counter() - t0, eng.nuts_stats()

    static(); nuts()
    st = [static() for _ in range(a.reps)]
    nt = [nuts() for _ in range(a.reps)]
    depth, nleap = eng.nuts_get_stats()
    got = eng.hmc_get(draws=False)
    ts, (rs, _) = float(np.median([w for w, _ in st])), st[0][1]
    tn, (rn, cn) = float(np.median([w for w, _ in nt])), nt[0][1]
    busy = int(np.sum(1 + nleap.sum(axis=1)))
    print(json.dumps({"d": d, "K": K, "J": a.J, "T": a.T, "max_depth": a.max_depth, "static_nleapfrog": a.nleapfrog, "static_rounds": rs,
                      "static_round_us": round(ts / rs * 1e6, 1), "nuts_rounds": rn, "nuts_rounds_issued": cn // K,
                      "nuts_round_us": round(tn / (cn // K) * 1e6, 1), "idle_share": round(1.0 - busy / cn, 4),
                      "transitions_per_s": round(K * a.T / tn, 1), "tree_depth": round(float(depth.mean()), 2),
                      "n_leapfrog": round(float(nleap.mean()), 2), "accept_prob": round(float(got["accept_prob"].mean()), 3),
                      "divergent": int(got["divergent"].sum()), "step_size": [round(float(eps.min()), 4), round(float(eps.max()), 4)]}))
    eng.close()


if __name__ == "__main__":
    main()
