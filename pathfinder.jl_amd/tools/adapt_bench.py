"""Device-resident warm-up (pfmi_hmc_adapt_enqueue / pfmi_nuts_adapt_enqueue) beside the window route (dual averaging on the host between
windows of 10 transitions: pfmi.hmc(adapt="windows")), in one process on the same fit, starts and seeds.

Shape: d = 1000, K = 64 chains, J = 6, the example HIP closure of examples/device_logp on t_lowrank(1000, 8, 2) (tools/nuts_bench.py's
setup), nwarmup = 200, then T sampling transitions.  Per sampler, the two routes INTERLEAVED (device, windows, device, ...), --reps pairs
after one unmeasured pair; one JSON line per sampler:
  * warmup_ms            host clock from the first enqueue to the end of the warm-up, [median, min, max] per route.  The device route has
                         no end of warm-up on the host, so it is the clock of an adaptive run with T = 1 sampling transition.
  * round_us             stage time per launch under pfmi_profile(2), [median, min, max] over the repetitions, three ways:
      same_work          the warm kernel against the plain kernel on IDENTICAL work: an adaptive run with nwarmup = 1 and N sampling
                         transitions against the plain calls that reproduce it bit for bit (one transition at eps_0, then CONTINUE with N
                         at the adaptive run's step sizes; the CONTINUE call is the one timed).  What differs is the kernel alone.
      warmup             the adaptive run of nwarmup transitions against ONE plain call of as many transitions at the adapted step
                         sizes: the same launch pattern (every chain works in every launch), other step sizes during the warm-up
      windows            the plain kernel inside the window route, where chains that have finished their window idle
  * accept               mean accept_prob of the T sampling transitions per route (target 0.8), and the step-size ranges
"""
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
        enq, wait = (eng.hmc_enqueue, eng.hmc_wait) if sampler == "hmc" else (eng.nuts_enqueue, eng.nuts_wait)
        aenq = eng.hmc_adapt_enqueue if sampler == "hmc" else eng.nuts_adapt_enqueue

        def windows(T):
            """(seconds of the warm-up, mean sampling acceptance, step sizes)"""
            t0 = time.perf_counter()
            eps, state, done = eps0, dual_averaging_init(eps0), 0
            while done < W:
                n = min(10, W - done)
                enq(pts, X0, seeds, eps, param, n, cont=done > 0)
                wait()
                done += n
                state, eps, ebar = dual_averaging_update(state, eng.hmc_get(draws=False)["accept_prob"].mean(axis=1), 0.8)
            t1 = time.perf_counter()
            eps = np.asarray(ebar)
            enq(pts, X0, seeds, eps, param, T, cont=True)
            wait()
            return t1 - t0, float(eng.hmc_get(draws=False)["accept_prob"].mean()), eps

        def device(T):
            t0 = time.perf_counter()
            aenq(pts, X0, seeds, eps0, param, W, T)
            wait()
            t1 = time.perf_counter()
            return t1 - t0, float(eng.hmc_get(draws=False)["accept_prob"].mean()), eng.adapt_get()["step_size"]

        device(1); windows(1)
        dv, wn = [], []
        for _ in range(a.reps):
            dv.append(device(1)[0]); wn.append(windows(1)[0])
        _, acc_d, eps_d = device(a.T)
        _, acc_w, eps_w = windows(a.T)
        # stage time per launch
        def stage(name, fn):
            m0, n0 = eng.kernel_time(name)
            fn()
            m1, n1 = eng.kernel_time(name)
            return (m1 - m0) / (n1 - n0) * 1e3, n1 - n0

        def adaptive_run(w, T):
            aenq(pts, X0, seeds, eps0, param, w, T)
            wait()

        def plain_run(eps, T, cont):
            enq(pts, X0, seeds, eps, param, T, cont=cont)
            wait()

        eng.profile(2)
        N = 4 * a.T
        adaptive_run(1, N)
        eps1 = eng.adapt_get()["step_size"]
        sw_a, sw_p, wu_a, wu_p, win_p, launches = [], [], [], [], [], {}
        for _ in range(a.reps):
            t, launches["same_work_adapt"] = stage(sampler + "_adapt", lambda: adaptive_run(1, N)); sw_a.append(t)
            plain_run(eps0, 1, False)
            t, launches["same_work_plain"] = stage(sampler, lambda: plain_run(eps1, N, True)); sw_p.append(t)
            t, launches["warmup_adapt"] = stage(sampler + "_adapt", lambda: adaptive_run(W, 1)); wu_a.append(t)
            t, launches["warmup_plain"] = stage(sampler, lambda: plain_run(eps_d, W + 1, False)); wu_p.append(t)
            t, _ = stage(sampler, lambda: windows(1)); win_p.append(t)
        eng.profile(0)
        stat = lambda v: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]     # noqa: E731
        print(json.dumps({"sampler": sampler, "d": d, "K": K, "nwarmup": W, "param": param, "reps": a.reps,
                          "warmup_ms": {"device": stat(np.array(dv) * 1e3), "windows": stat(np.array(wn) * 1e3)},
                          "round_us": {"same_work": {"adapt": stat(sw_a), "plain": stat(sw_p)}, "warmup": {"adapt": stat(wu_a), "plain": stat(wu_p)},
                                       "windows": {"plain": stat(win_p)}, "launches": launches},
                          "accept": {"device": round(acc_d, 3), "windows": round(acc_w, 3), "target": 0.8},
                          "step_size": {"device": [round(float(eps_d.min()), 4), round(float(eps_d.max()), 4)],
                                        "windows": [round(float(eps_w.min()), 4), round(float(eps_w.max()), 4)]}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
