"""Time the low-rank route to the pooled covariance's top eigenpairs (pfmi_pool_apply, MultiPathfinderResult.lowrank_covariance) against
the dense route (covariance() followed by numpy.linalg.eigh).

    python tools/pool_apply_bench.py [--configs 1000:64:1000:16,10000:32:1000:16] [--reps 5] [--dense-max-d 10000] [--out FILE]

A config is d:K:N_r:rank.  A multipathfinder run (nruns = K, ndraws_per_run = N_r, 30 L-BFGS iterations) provides the result; per config
one JSON object:
  scores_ms, apply_ms, combine_ms   the three kernels of one pfmi_pool_apply with r = rank directions (hipEvent pairs in the stream,
                                    pfmi_kernel_time), mean of --reps after one warm-up call
  pool_bytes, scores_bytes          what one launch has to move at least: both kernels read the pool once; the scores kernel writes and
                                    the apply kernel reads K N_r r doubles
  scores_tbs, apply_tbs             (pool_bytes + scores_bytes) / kernel time, in 1e12 bytes per second
  apply_call_ms                     Engine.pool_apply end to end: uploads of the centre and the directions, the kernels, download of Y
  lowrank_ms, passes, converged,    wall clock of result.lowrank_covariance(rank) (median of --reps: pool rebuild, PSIS, two moment passes
  block                             and `passes` applications of a block of `block` directions) and what the iteration reports
  covariance_ms, eigh_ms            the dense route on the same result: result.covariance() and numpy.linalg.eigh of its cov (skipped
                                    above --dense-max-d: null)
  max_rel_eig_diff                  max_j |lam_j - eigh's| / lam_1 over the rank returned values where the dense route ran
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _kernel_ms(eng, names, call, reps):
    call()                                                          # warm-up
    eng.profile(2)
    before = {n: eng.kernel_time(n) for n in names}
    for _ in range(reps):
        call()
    after = {n: eng.kernel_time(n) for n in names}
    eng.profile(0)
    return {n: (after[n][0] - before[n][0]) / max(after[n][1] - before[n][1], 1) for n in names}


def _median_ms(call, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def run(pfmi, d, K, N_r, rank, reps, dense_max_d):
    tg = pfmi.t_lowrank(d, r=8, seed=2)
    eng = pfmi.Engine(0)
    res = pfmi.multipathfinder(tg, 100, nruns=K, ndraws_per_run=N_r, rng=pfmi.HostRNG(4), engine=eng, maxiters=30)
    lr = res.lowrank_covariance(rank)                               # warm-up; leaves the pool and its PSIS weights on the engine
    V = np.ascontiguousarray(lr.eigenvectors.T)
    km = _kernel_ms(eng, ["pool_scores", "pool_apply", "pool_apply_combine"], lambda: eng.pool_apply(0, True, lr.mean, V), reps)
    apply_call_ms, _ = _median_ms(lambda: eng.pool_apply(0, True, lr.mean, V), reps)
    lowrank_ms, lr = _median_ms(lambda: res.lowrank_covariance(rank), reps)
    pool_bytes, scores_bytes = 8 * d * K * N_r, 8 * K * N_r * rank
    covariance_ms = eigh_ms = rel = None
    if d <= dense_max_d:
        res.covariance()                                            # warm-up (allocates the d x d buffer)
        covariance_ms, c = _median_ms(lambda: res.covariance(), max(1, reps // 2))
        t0 = time.perf_counter()
        ev = np.linalg.eigh(c.cov)[0]
        eigh_ms = (time.perf_counter() - t0) * 1e3
        rel = float(np.max(np.abs(ev[::-1][:rank] - lr.eigenvalues)) / ev[-1])
    eng.close()
    return dict(d=d, K=K, N_r=N_r, rank=rank, block=int(min(d, 32, rank + 8)), pool_bytes=pool_bytes, scores_bytes=scores_bytes,
                scores_ms=km["pool_scores"], apply_ms=km["pool_apply"], combine_ms=km["pool_apply_combine"],
                scores_tbs=(pool_bytes + scores_bytes) / (km["pool_scores"] * 1e-3) / 1e12,
                apply_tbs=(pool_bytes + scores_bytes) / (km["pool_apply"] * 1e-3) / 1e12, apply_call_ms=apply_call_ms,
                lowrank_ms=lowrank_ms, passes=lr.passes, converged=lr.converged, covariance_ms=covariance_ms, eigh_ms=eigh_ms,
                max_rel_eig_diff=rel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000:64:1000:16,10000:32:1000:16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-max-d", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pfmi
    rows = []
    for cfg in a.configs.split(","):
        d, K, N_r, rank = (int(x) for x in cfg.split(":"))
        rows.append(run(pfmi, d, K, N_r, rank, a.reps, a.dense_max_d))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
