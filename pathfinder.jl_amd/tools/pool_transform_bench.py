"""Time one pfmi_pool_transform pass against the pfmi_pool_moments pass over the same pool, the whole moment_match call against what
a user has without it (download the pool, move it on the host, re-evaluate), and record k-hat before and after.

    python tools/pool_transform_bench.py [--config 1000:64:1000] [--reps 20] [--targets headline,fitted] [--out FILE]

A config is d:K:N_r.  Per target one JSON object:
  transform_ms, ratio_ms       the transform pass and its ratio kernel (hipEvent pairs in the stream, pfmi_kernel_time), mean of --reps
  moments_ms                   the moment kernel + its chunk-sum kernel over the same pool, same session, same method
  transform_over_moments       (transform_ms + ratio_ms) / moments_ms: the pass moves 16 d S bytes, the moment pass reads 8 d S
  moved_GBps                   16 d S bytes over transform_ms
  call_ms                      Engine.pool_transform(want=False) end to end, median
  host_ms                      the alternative: pool_get, scale x + shift with NumPy, logp of the target on the host (pool upload not counted)
  moment_match_ms              result.moment_match() end to end; khat_before, khat_after, history: what it did
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _kt(eng, names):
    return [eng.kernel_time(n) for n in names]


def run(pfmi, name, d, K, N_r, reps):
    tg = pfmi.t_lowrank(d, r=8, seed=2, wscale=(1.0 if name == "headline" else 2 / np.sqrt(d)))
    eng = pfmi.Engine(0)
    t0 = time.perf_counter()
    res = pfmi.multipathfinder(tg, 1000, nruns=K, ndraws_per_run=N_r, rng=pfmi.HostRNG(4), engine=eng)
    mpf_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(1)
    scale, shift = 0.9 + 0.2 * rng.random(d), 0.1 * rng.normal(size=d)
    pfmi.api._rebuild_pool(res, True)                             # the pool and its weights, as every summary leaves them
    names = ("pool_transform", "pool_transform_ratio", "pool_moments", "pool_moments_sum")
    eng.pool_transform(scale, shift, want=False)                  # warm-up (allocates the spare sets)
    eng.pool_moments(0, True, None)
    eng.profile(2)
    a = _kt(eng, names)
    for _ in range(reps):
        eng.pool_transform(scale, shift, want=False)
        eng.pool_moments(0, True, None)
    b = _kt(eng, names)
    eng.profile(0)
    ms = [(y[0] - x[0]) / max(y[1] - x[1], 1) for x, y in zip(a, b)]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.pool_transform(scale, shift, want=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.pool_transform(None, None, want=False)
    t0 = time.perf_counter()
    P, _ = eng.pool_get()
    X = scale[:, None] * np.asarray(P).reshape(d, -1, order="F") + shift[:, None]
    tg.logp(X)
    host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    mr = res.moment_match()
    mm_ms = (time.perf_counter() - t0) * 1e3
    eng.close()
    S = K * N_r
    return dict(target=name, d=d, K=K, N_r=N_r, transform_ms=ms[0], ratio_ms=ms[1], moments_ms=ms[2] + ms[3],
                transform_over_moments=(ms[0] + ms[1]) / (ms[2] + ms[3]), moved_GBps=16.0 * d * S / (ms[0] * 1e-3) / 1e9,
                call_ms=float(np.median(ts)), host_ms=host_ms, multipathfinder_ms=mpf_ms, moment_match_ms=mm_ms,
                khat_before=res.psis_result.pareto_shape, khat_after=mr.psis_result.pareto_shape,
                history=[(s, round(k, 4), bool(acc)) for s, k, acc in mr.moment_match_history])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1000:64:1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--targets", default="headline,fitted")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pfmi
    d, K, N_r = (int(x) for x in a.config.split(":"))
    rows = []
    for name in a.targets.split(","):
        rows.append(run(pfmi, name, d, K, N_r, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
