"""Fused NUTS on a built-in target (pfmi_nuts_fused_enqueue: one workgroup per chain builds its trees at its own pace over the trips of a
launch) beside the only route the same chains had before it: pfmi_nuts_enqueue on the example HIP closure of examples/device_logp that
restates the same density (one closure call and one step launch per round, every chain's workgroup launched until the slowest chain is
done).  One process, the two routes INTERLEAVED.

Shape: t_lowrank(1000, r=8), J = 6, max_depth 8, T = 200, K = 64, 256 and 1024 chains, every chain on the best fit of one path from that
fit's trace point, step size d^(-1/4), the same seeds on both routes.  One unmeasured pair, then --reps pairs; one JSON line per K:
  * wall_ms        HOST clock from the enqueue to the return of nuts_wait, [median, min, max] per route
  * stage_ms       DEVICE-EVENT time under pfmi_profile(2), in runs of their own, [median, min, max]: the "nuts_fused" stage of the fused
                   route; "nuts" + "nuts_closure" of the rounds route (its launches: two per round)
  * us_per_step    wall_ms / (leapfrog steps of all chains): microseconds per leapfrog step and chain (HOST clock)
  * speedup        rounds wall / fused wall (medians); wins: the fused [min, max] lies wholly below the rounds route's
  * depth, accept  mean tree depth and acceptance of each route (the two restate one density: they must agree)
then one line for the launch cap (PFMI_NUTS_FUSED_ROUNDS) at --cap-K chains: wall_ms of the fused route at caps 1, 64, 1024 and uncut,
interleaved, with the launches each made, and whether 1024 (csrc/hmc_rows.h: HM_FUSED_ROUNDS, shared with fused static HMC) lies inside
the uncut run's min-to-max spread.
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
from hmc_fused_bench import setup, stat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap-K", type=int, default=64)
    ap.add_argument("--caps", type=int, nargs="+", default=[1, 64, 1024, 0], help="0: uncut")
    a = ap.parse_args()
    d, T, md = a.d, a.T, a.max_depth
    tg = pfmi.t_lowrank(d, a.r, 2)
    L = pfmi._lib.lib()
    fe, ce = pfmi.Engine(0), pfmi.Engine(0)                    # the built-in target; the closure that restates it
    eps = d ** -0.25

    def cap(n):
        L.pfmi_debug_set(b"PFMI_NUTS_FUSED_ROUNDS", None if n is None else str(n if n else 2 ** 31 - 1).encode())

    def timed(eng, enqueue, stages):
        m0 = [eng.kernel_time(s) for s in stages]
        t0 = time.perf_counter()
        enqueue()
        eng.nuts_wait()
        t1 = time.perf_counter()
        m1 = [eng.kernel_time(s) for s in stages]
        return (t1 - t0) * 1e3, sum(b[0] - a_[0] for a_, b in zip(m0, m1)), sum(b[1] - a_[1] for a_, b in zip(m0, m1))

    def trees(eng):
        dep, nl = eng.nuts_get_stats()
        return float(dep.mean()), int(nl.sum()), float(eng.hmc_get(draws=False)["accept_prob"].mean())

    try:
        for K in a.K:
            fp, fx = setup(fe, tg, d, a.J, K)
            cp, cx = setup(ce, hip_target(tg), d, a.J, K)
            seeds = pfmi.HostRNG(17).rand_u64(K)
            fused = lambda: fe.nuts_fused_enqueue(fp, fx, seeds, eps, md, T)                      # noqa: E731
            rounds = lambda: ce.nuts_enqueue(cp, cx, seeds, eps, md, T)                           # noqa: E731
            timed(fe, fused, ()); timed(ce, rounds, ())
            wf, wr, sf, sr_, nf, nr = [], [], [], [], 0, 0
            for _ in range(a.reps):
                wf.append(timed(fe, fused, ())[0]); wr.append(timed(ce, rounds, ())[0])
            (fdep, fsteps, facc), (cdep, csteps, cacc) = trees(fe), trees(ce)
            fstats, cstats = fe.nuts_stats(), ce.nuts_stats()
            fe.profile(2); ce.profile(2)
            for _ in range(a.reps):
                _, ms, nf = timed(fe, fused, ("nuts_fused",)); sf.append(ms)
                _, ms, nr = timed(ce, rounds, ("nuts", "nuts_closure")); sr_.append(ms)
            fe.profile(0); ce.profile(0)
            print(json.dumps({"K": K, "d": d, "r": a.r, "J": a.J, "T": T, "max_depth": md, "reps": a.reps, "step_size": round(eps, 4),
                              "wall_ms": {"fused": stat(wf), "rounds": stat(wr), "clock": "host"},
                              "stage_ms": {"fused": stat(sf), "rounds": stat(sr_), "clock": "device events", "launches": {"fused": nf, "rounds": nr}},
                              "us_per_step": {"fused": round(float(np.median(wf)) * 1e3 / fsteps, 4), "rounds": round(float(np.median(wr)) * 1e3 / csteps, 4)},
                              "speedup": round(float(np.median(wr) / np.median(wf)), 2), "fused_wins": bool(max(wf) < min(wr)),
                              "depth": [round(fdep, 3), round(cdep, 3)], "accept": [round(facc, 3), round(cacc, 3)],
                              "leapfrog_steps": [fsteps, csteps], "trips_of_the_slowest_chain": [fstats[0], cstats[0]]}), flush=True)
        K = a.cap_K
        fp, fx = setup(fe, tg, d, a.J, K)
        seeds = pfmi.HostRNG(17).rand_u64(K)
        fused = lambda: fe.nuts_fused_enqueue(fp, fx, seeds, eps, md, T)                          # noqa: E731
        plan = "nuts_fused:%d:%s:g%d" % (12 if a.J == 6 else 0, "res", 8 if 0 < a.r <= 8 else (16 if a.r else 0))
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
        out = {"caps": {("uncut" if c == 0 else str(c)): {"wall_ms": stat(walls[c]), "launches": launches[c]} for c in a.caps}, "K": K,
               "trips_of_the_slowest_chain": fe.nuts_stats()[0], "clock": "host", "plan": plan}
        if 0 in walls and 1024 in walls:
            out["cap_1024_inside_uncut_spread"] = bool(min(walls[0]) <= float(np.median(walls[1024])) <= max(walls[0]))
        print(json.dumps(out), flush=True)
    finally:
        cap(None)
        fe.close(); ce.close()


if __name__ == "__main__":
    main()
