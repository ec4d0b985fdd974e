"""Fused static HMC on a built-in target (pfmi_hmc_fused_enqueue: one workgroup per chain loops over the rounds of a launch) beside the
only route the same chains had before it: pfmi_hmc_enqueue on the example HIP closure of examples/device_logp that restates the same
density (one closure call and one step launch per round).  One process, the two routes INTERLEAVED.

Shape: t_lowrank(1000, r=8), J = 6, Lf = 8, T = 200 (1601 rounds), K = 64, 256 and 1024 chains, every chain on the best fit of one path
from that fit's trace point, step size 0.5 d^(-1/4), the same seeds on both routes.  One unmeasured pair, then --reps pairs; one JSON
line per K:
  * wall_ms        HOST clock from the enqueue to the return of hmc_wait, [median, min, max] per route
  * stage_ms       DEVICE-EVENT time under pfmi_profile(2), [median, min, max]: the "hmc_fused" stage of the fused route; "hmc" +
                   "hmc_closure" of the rounds route (its launches: two per round)
  * us_per_step    wall_ms / (T Lf K): microseconds per leapfrog step and chain (HOST clock)
  * speedup        rounds wall / fused wall (medians)
then one line for the launch cap (PFMI_HMC_FUSED_ROUNDS) at --cap-K chains: wall_ms of the fused route at caps 1, 64, 1024 and uncut,
interleaved, with the launches each made.  The shipped cap (csrc/hmc_rows.h: HM_FUSED_ROUNDS) is the smallest whose time lies within
the run-to-run spread of the uncut run.
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


def setup(eng, target, d, J, K):
    """one path, its best fit; K chains on that fit from its trace point"""
    eng.set_target(target)
    npts = eng.optimize_batch(pfmi.HostRNG(3).rand(d).reshape(1, d) * 4 - 2, J, 200, 1e-8)
    eng.fit_batch(J)
    _, _, best = eng.elbo_batch(64, pfmi.hostrng.rand_u64(5, np.arange(int(npts[0]), dtype=np.uint64), 9))
    p = int(best[0])
    th, _, _ = eng.get_trace(0)
    return np.full(K, p, dtype=np.int64), np.asfortranarray(np.repeat(th[p][:, None], K, axis=1))


def stat(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--nleapfrog", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap-K", type=int, default=64)
    ap.add_argument("--caps", type=int, nargs="+", default=[1, 64, 1024, 0], help="0: uncut")
    a = ap.parse_args()
    d, T, Lf = a.d, a.T, a.nleapfrog
    tg = pfmi.t_lowrank(d, a.r, 2)
    L = pfmi._lib.lib()
    fe, ce = pfmi.Engine(0), pfmi.Engine(0)                    # the built-in target; the closure that restates it
    eps = 0.5 * d ** -0.25

    def cap(n):
        L.pfmi_debug_set(b"PFMI_HMC_FUSED_ROUNDS", None if n is None else str(n if n else 2 ** 31 - 1).encode())

    def timed(eng, enqueue, stages):
        m0 = [eng.kernel_time(s) for s in stages]
        t0 = time.perf_counter()
        enqueue()
        eng.hmc_wait()
        t1 = time.perf_counter()
        m1 = [eng.kernel_time(s) for s in stages]
        return (t1 - t0) * 1e3, sum(b[0] - a_[0] for a_, b in zip(m0, m1)), sum(b[1] - a_[1] for a_, b in zip(m0, m1))

    try:
        for K in a.K:
            fp, fx = setup(fe, tg, d, a.J, K)
            cp, cx = setup(ce, hip_target(tg), d, a.J, K)
            seeds = pfmi.HostRNG(17).rand_u64(K)
            fused = lambda: fe.hmc_fused_enqueue(fp, fx, seeds, eps, Lf, T)                       # noqa: E731
            rounds = lambda: ce.hmc_enqueue(cp, cx, seeds, eps, Lf, T)                             # noqa: E731
            timed(fe, fused, ()); timed(ce, rounds, ())
            wf, wr, sf, sr_, nf, nr = [], [], [], [], 0, 0
            for _ in range(a.reps):
                wf.append(timed(fe, fused, ())[0]); wr.append(timed(ce, rounds, ())[0])
            acc = (float(fe.hmc_get(draws=False)["accept_prob"].mean()), float(ce.hmc_get(draws=False)["accept_prob"].mean()))
            fe.profile(2); ce.profile(2)
            for _ in range(a.reps):
                _, ms, nf = timed(fe, fused, ("hmc_fused",)); sf.append(ms)
                _, ms, nr = timed(ce, rounds, ("hmc", "hmc_closure")); sr_.append(ms)
            fe.profile(0); ce.profile(0)
            per = 1e3 / (T * Lf * K)
            print(json.dumps({"K": K, "d": d, "r": a.r, "J": a.J, "T": T, "nleapfrog": Lf, "reps": a.reps, "step_size": round(eps, 4),
                              "wall_ms": {"fused": stat(wf), "rounds": stat(wr), "clock": "host"},
                              "stage_ms": {"fused": stat(sf), "rounds": stat(sr_), "clock": "device events", "launches": {"fused": nf, "rounds": nr}},
                              "us_per_step": {"fused": round(float(np.median(wf)) * per, 4), "rounds": round(float(np.median(wr)) * per, 4)},
                              "speedup": round(float(np.median(wr) / np.median(wf)), 2), "accept": [round(x, 3) for x in acc]}), flush=True)
        K = a.cap_K
        fp, fx = setup(fe, tg, d, a.J, K)
        seeds = pfmi.HostRNG(17).rand_u64(K)
        fused = lambda: fe.hmc_fused_enqueue(fp, fx, seeds, eps, Lf, T)                           # noqa: E731
        plan = "hmc_fused:%d:%s:g%d" % (12 if a.J == 6 else 0, "res", 8 if 0 < a.r <= 8 else (16 if a.r else 0))
        walls, launches = {c: [] for c in a.caps}, {}
        for c in a.caps:
            cap(c); timed(fe, fused, ())
        for _ in range(a.reps):
            for c in a.caps:
                cap(c)
                n0 = fe.kernel_time(plan)[1]
                walls[c].append(timed(fe, fused, ())[0])
                launches[c] = fe.kernel_time(plan)[1] - n0
        cap(None)
        print(json.dumps({"caps": {("uncut" if c == 0 else str(c)): {"wall_ms": stat(walls[c]), "launches": launches[c]} for c in a.caps}, "K": K,
                          "rounds": 1 + T * Lf, "clock": "host", "plan": plan}), flush=True)
    finally:
        cap(None)
        fe.close(); ce.close()


if __name__ == "__main__":
    main()
