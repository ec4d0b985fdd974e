"""Time the CDF pass over the pool (pfmi_pool_cdf) and the quantile search on it (pfmi.importance_quantiles' _quantile_search) against
a device-to-device copy of as many bytes and against what a user has without it (download the pool, sort with NumPy).

    python tools/pool_quantiles_bench.py [--configs 1000:64:1000,10000:32:1000] [--reps 5] [--out FILE]

A config is d:K:N_r.  Per config one JSON object:
  pass_ms                     {nthr: ms} of one CDF pass at nthr = 4, 8, 16, 32 thresholds: the CDF kernel plus the combine kernel
                              (hipEvent pairs in the stream, pfmi_kernel_time), mean of --reps
  read_GBps                   {nthr: pool bytes (8 d K N_r) per second of that pass}
  copy_ms, copy_GBps          torch copy of a device buffer of pool_bytes into another; the rate counts the bytes once
  read_vs_copy                {nthr: read_GBps / copy_GBps}
  call_ms                     {nthr: Engine.pool_cdf end to end: upload of the thresholds, both kernels, download of 3 nthr d numbers}
  search                      {thresholds per pass: [passes, total ms]} of the bracket search alone (_quantile_search on the pool as
                              built and weighted, W given) for the five default probabilities under the PSIS weights
  quantiles_of_pool           [passes, ms] of importance_quantiles after its preamble (the moment pass for W + the search at the
                              default thresholds per pass); the preamble -- the pool rebuild and the pooled PSIS that summary() also
                              performs -- needs a multipathfinder result and is not timed here
  pool_get_ms, numpy_ms       the alternative: Engine.pool_get() of the draws, then a stable argsort and a cumulative weight sum per row
  equal_to_numpy              every searched quantile equals the host's
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

PROBS = np.array([0.025, 0.25, 0.5, 0.75, 0.975])


def _numpy_quantiles(P2, w, W):
    """the definition of include/pfmi.h in float64 on the host: per row a stable argsort and the cumulative weights"""
    keep = w != 0.0
    X, wk = P2[:, keep], w[keep]
    out = np.empty((PROBS.size, X.shape[0]))
    for i in range(X.shape[0]):
        o = np.argsort(X[i], kind="stable")
        xs, cw = X[i][o], np.cumsum(wk[o])
        last = np.concatenate([xs[1:] != xs[:-1], [True]])
        vals, U = xs[last], cw[last]
        out[:, i] = vals[np.minimum(np.searchsorted(U, PROBS * W, side="left"), vals.size - 1)]
    return out


def run(pfmi, torch, d, K, N_r, reps, J=6):
    from pfmi.api import _combine_moments, _quantile_search, _quantiles_of_pool
    tg = pfmi.t_lowrank(d, r=8, seed=2)
    eng = pfmi.Engine(0)
    eng.set_target(tg)
    x0 = pfmi.HostRNG(11).rand(K * d).reshape(K, d) * 4 - 2
    eng.optimize_batch(x0, J, 30)
    eng.fit_batch(J)
    pts = [int(eng.offsets[k + 1]) - 1 for k in range(K)]
    eng.pool_build(N_r, pts, np.arange(1, K + 1, dtype=np.uint64))
    _, lr = eng.pool_get(draws=False)
    w = eng.psis(lr)["weights"]
    nbytes = 8 * d * K * N_r
    mean = np.asarray(tg.mean, dtype=np.float64)
    T32 = mean[None, :] + np.linspace(-2.0, 2.0, 32)[:, None]

    pass_ms, call_ms = {}, {}
    for nthr in (4, 8, 16, 32):
        T = T32[:nthr]
        eng.pool_cdf(0, True, T)                                  # warm-up
        eng.profile(2)
        m0, n0 = eng.kernel_time("pool_cdf")
        s0, _ = eng.kernel_time("pool_cdf_combine")
        for _ in range(reps):
            eng.pool_cdf(0, True, T)
        m1, n1 = eng.kernel_time("pool_cdf")
        s1, _ = eng.kernel_time("pool_cdf_combine")
        eng.profile(0)
        pass_ms[nthr] = ((m1 - m0) + (s1 - s0)) / max(n1 - n0, 1)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.pool_cdf(0, True, T)
            ts.append((time.perf_counter() - t0) * 1e3)
        call_ms[nthr] = float(np.median(ts))

    W = _combine_moments([eng.pool_moments(0, True, None)[0]])[0]
    search, answers = {}, {}
    for per_pass in (10, 20, 30):
        t0 = time.perf_counter()
        q, passes = _quantile_search(lambda T: eng.pool_cdf(0, True, T), d, PROBS * W, per_pass // PROBS.size)
        search[per_pass] = [passes, (time.perf_counter() - t0) * 1e3]
        answers[per_pass] = q

    _quantiles_of_pool([eng], [(0, K)], N_r, True, PROBS)
    t0 = time.perf_counter()
    qd, pd = _quantiles_of_pool([eng], [(0, K)], N_r, True, PROBS)
    of_pool = [pd, (time.perf_counter() - t0) * 1e3]
    answers["default"] = qd

    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda:0").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / reps
    del src, dst

    t0 = time.perf_counter()
    P, _ = eng.pool_get()
    pool_get_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = _numpy_quantiles(P.reshape(d, K * N_r, order="F"), w, W)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    eng.close()
    copy = nbytes / (copy_ms * 1e-3) / 1e9
    read = {n: nbytes / (ms * 1e-3) / 1e9 for n, ms in pass_ms.items()}
    return dict(d=d, K=K, N_r=N_r, pool_bytes=nbytes, pass_ms=pass_ms, read_GBps=read, copy_ms=copy_ms, copy_GBps=copy,
                read_vs_copy={n: r / copy for n, r in read.items()}, call_ms=call_ms, search=search, quantiles_of_pool=of_pool, pool_get_ms=pool_get_ms,
                numpy_ms=numpy_ms, equal_to_numpy={n: bool(np.array_equal(q, ref)) for n, q in answers.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000:64:1000,10000:32:1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pfmi
    rows = []
    for cfg in a.configs.split(","):
        d, K, N_r = (int(x) for x in cfg.split(":"))
        rows.append(run(pfmi, torch, d, K, N_r, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
